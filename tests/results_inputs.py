"""Small inputs of the results stage with the edges planted (tests/test_results_twin.py, tests/test_gpu_results.py).

Sizes are the smallest at which a structure exists: one row, two, either side of a wave (64) and of a workgroup (1024), two and four
workgroups and a row, the sizes at which (n - 1) theta is an integer for every quantile (n - 1 a multiple of 980, no zero baseMean), and
3 * 1024 + 7 rows whose p-values below alpha end at a workgroup's edge.  The one large input is the IHW case of 262 145 rows (one row
beyond one grid-stride trip of the group kernel), with two groups and four distinct distances.

baseMean is tied the way counts tie it: a few hundred distinct multiples of 1/8, runs of equal values across the quantile positions.

HOW THE BH EDGE IS PLANTED (`edge` cases).  R rows carry the largest baseMean, so they pass every filter, and the R smallest p-values,
so the row of rank r has rank r under every filter; every other p-value lies above alpha and can reject nothing.  Rank r is given the
double nearest alpha r / m_f(r) or one of its neighbours, m_f the rows filter f keeps, with f(r) increasing in r: under filter f the
ranks behind f's own were planted for a smaller m and fail, so f's own planted rank IS the decision numRej[f] hangs on.  Among the
three candidates the one on which fl(fl(m / r) p) < alpha and the exact m p / r < alpha disagree is taken where there is one.

HOW numRej PROFILES ARE STEERED (`steps` cases).  The same R rows with p_r = r q: q below alpha / m_f exactly for f >= f0 gives
numRej = 0 before f0 and R from f0 on — a single point (f0 = 49), a plateau (R = 10 and 11: either side of the `max(numRej) <= 10` rule; 12), a constant profile (f0 = 0:
its lowess residuals are zero).
"""
import math
from fractions import Fraction

import numpy as np

import results_exact_twin as rx

NAN = float("nan")


# ---------------------------------------------------------------------------------------------------------------------------
# independent filtering
# ---------------------------------------------------------------------------------------------------------------------------
def tied_basemean(n, rng, zeros=0, integer=False, distinct=300):
    """count-like: values k / 8 (or k), geometric-ish frequencies, `zeros` rows of exactly 0 and none besides"""
    k = np.minimum(rng.geometric(0.02, n), 40 * distinct // 8) + rng.integers(0, 3, n)
    k = 1 + (k % distinct)
    bm = k.astype(float) if integer else k / 8.0
    bm[rng.choice(n, zeros, replace=False)] = 0.0
    return bm


def natural_p(bm, rng):
    """many small p-values among the rows of large baseMean: numRej rises with the filter, then falls"""
    hi = bm > np.median(bm)
    return rng.uniform(size=len(bm)) ** np.where(hi, 7.0, 1.0)


def _m_of(bm, p):
    """rows each filter keeps (with a p-value), from the exact cuts; None where the cut has a band"""
    c = rx.cuts(bm)
    ok = ~np.isnan(p)
    fb = [Fraction(float(v)) for v in bm]
    return [None if c["band"][f] else sum(1 for v, o in zip(fb, ok) if o and v >= c["cut"][f]) for f in range(rx.NQ)], c


def plant_edge(bm, p, alpha, R, rng):
    """see the module's docstring; returns the planted (row, rank, filter, m, which neighbour)"""
    n = len(bm)
    rows = rng.choice(n, R, replace=False)
    bm[rows] = bm.max() + 1.0
    p[:] = np.where(np.isnan(p), p, alpha + (1.0 - alpha) * rng.uniform(size=n) ** 2 + 1e-9)
    p[p > 1.0] = 1.0
    p[rows] = 0.5
    m, _ = _m_of(bm, p)
    usable = [f for f in range(rx.NQ) if m[f] is not None and m[f] >= R]
    fs = sorted(usable[int(round(t))] for t in np.linspace(0, len(usable) - 1, R))
    planted, a, A = [], float(alpha), Fraction(float(alpha))
    for r, (row, f) in enumerate(zip(rows, fs), start=1):
        centre = float(A * r / m[f])
        cand = [centre, math.nextafter(centre, 0.0), math.nextafter(centre, 1.0)]
        differ = [c for c in cand if ((m[f] / r) * c < a) != (Fraction(m[f], r) * Fraction(c) < A)]
        equal = [c for c in cand if (m[f] / r) * c == a]          # fl(fl(m / r) p) == alpha: `<` and `<=` part here
        prefer = (equal + differ) if r % 2 else (differ + equal)
        p[row] = prefer[0] if prefer else cand[r % 3]
        planted.append((int(row), r, f, m[f], cand.index(p[row])))
    assert np.all(np.diff(p[rows]) > 0) and p[rows].max() <= alpha * (1 + 1e-12)
    return planted


def plant_steps(bm, p, alpha, R, f0, rng):
    n = len(bm)
    rows = rng.choice(n, R, replace=False)
    bm[rows] = bm.max() + 1.0
    p[:] = np.where(np.isnan(p), p, alpha + (1.0 - alpha) * rng.uniform(size=n) + 1e-9)
    p[p > 1.0] = 1.0
    p[rows] = 0.5
    m, _ = _m_of(bm, p)
    assert m[f0] is not None and (f0 == 0 or (m[f0 - 1] is not None and m[f0 - 1] > m[f0]))
    q = alpha / m[f0] * (1 - 1e-6) if f0 == 0 else 0.5 * (alpha / m[f0 - 1] + alpha / m[f0])
    p[rows] = q * np.arange(1, R + 1)


IF_CASES = ["n1", "n2", "n63-edge", "n64-integer-edge-a05", "n65-constant", "n1023-zeros-na", "n1024-lower-under", "n1025-lower-over",
            "n2049-lower-one", "n4097-edge", "n4097-ties", "n981-integer-h", "n1961-integer-h", "n4901-integer-h-a05",
            "n3079-exit-1024", "n3079-exit-1025", "n3079-exit-2048", "n1023-all-below", "n1023-max10", "n1023-max11", "n1023-constant11",
            "n1023-all-zero", "n1023-single-point", "n1023-plateau"]
_if_cache = {}


def if_case(name):
    if name in _if_cache:
        return _if_cache[name]
    rng = np.random.default_rng(3200 + sum(map(ord, name)))
    n = int(name.split("-")[0][1:])
    alpha = 0.05 if name.endswith("a05") else 0.1
    planted = []
    if name == "n1":
        bm, p = np.array([3.5]), np.array([0.01])
    elif name == "n2":
        bm, p = np.array([0.0, 2.0]), np.array([0.04, NAN])
    elif "edge" in name:
        bm = tied_basemean(n, rng, zeros=n // 10, integer="integer" in name)
        p = rng.uniform(size=n)
        p[rng.choice(n, n // 20, replace=False)] = NAN
        planted = plant_edge(bm, p, alpha, {63: 3, 64: 3, 4097: 40}[n], rng)
    elif name == "n65-constant":
        bm = np.full(n, 2.625)
        p = rng.uniform(size=n) ** 6
    elif name == "n1023-zeros-na":
        bm = tied_basemean(n, rng, zeros=300)
        p = natural_p(bm, rng)
        top = np.flatnonzero(bm >= np.quantile(bm, 0.97))
        p[top[::2]] = NAN                               # pass every filter, no p-value
        p[np.flatnonzero(bm == 0)[::3]] = 1e-9          # a p-value, baseMean 0
        p[np.flatnonzero(bm == 0)[1::3]] = NAN
    elif name in ("n1024-lower-under", "n1025-lower-over"):
        bm = tied_basemean(n, rng, zeros=972 if n == 1024 else 974)
        p = natural_p(bm, rng) ** 2
    elif name == "n2049-lower-one":
        bm = np.zeros(n)
        p = rng.uniform(size=n) ** 5
    elif name == "n4097-ties":
        bm = tied_basemean(n, rng, zeros=50)
        p = 0.2 + 0.8 * rng.uniform(size=n)
        order = rng.permutation(n)
        p[order[:70]] = 0.0                             # ties at 0 across the first wave edge
        p[order[70:1100]] = 0.015625                    # one run across wave edges and the first workgroup edge
        p[order[1100:1400]] = 1.0
        p[order[1400:1500]] = NAN
    elif "integer-h" in name:
        bm = tied_basemean(n, rng, zeros=0)
        p = natural_p(bm, rng)
    elif "exit" in name:
        K = int(name.split("-")[-1])
        bm = tied_basemean(n, rng, zeros=100)
        p = alpha + (1 - alpha) * rng.uniform(size=n) + 1e-9
        p[p > 1.0] = 1.0
        order = rng.permutation(n)
        p[order[:K]] = alpha * rng.uniform(size=K) ** 3
        p[order[K]] = alpha                             # the key the early exit compares with, exactly
        p[order[K - 1]] = math.nextafter(alpha, 0.0)
    elif name == "n1023-all-below":
        bm = tied_basemean(n, rng, zeros=40)
        p = alpha * rng.uniform(size=n) ** 2 * 0.999
    else:
        bm = tied_basemean(n, rng, zeros=100)
        p = rng.uniform(size=n)
        R, f0 = {"max10": (10, 30), "max11": (11, 30), "constant11": (11, 0), "all-zero": (0, 0), "single-point": (11, 49), "plateau": (12, 30)}[name.split("-", 1)[1]]
        plant_steps(bm, p, alpha, R, f0, rng)
    case = dict(name=name, baseMean=np.ascontiguousarray(bm, dtype=np.float64), pvalue=np.ascontiguousarray(p, dtype=np.float64), alpha=alpha,
                planted=planted)
    _if_cache[name] = case
    return case


# ---------------------------------------------------------------------------------------------------------------------------
# Cook's filter
# ---------------------------------------------------------------------------------------------------------------------------
COOKS_DESIGNS = {"S3-000": "000", "S4-0011": "0011", "S5-00111": "00111", "S8-4v4": "0" * 4 + "1" * 4, "S64-32v32": "0" * 32 + "1" * 32}
COOKS_N = 300   # more than one block of 256
_cooks_cache = {}


def cooks_case(name):
    if name in _cooks_cache:
        return _cooks_cache[name]
    group = np.array([int(c) for c in COOKS_DESIGNS[name]], dtype=np.int32)
    S = len(group)
    m, p, applies = rx.design(group)
    rng = np.random.default_rng(3210 + S)
    cutoff = float(rx.qf99(p, m - p)) if m > p else 1.0
    counts = rng.integers(0, 6 if S <= 8 else 40, (COOKS_N, S)).astype(np.int32)   # small: ties with the flagged count in most rows
    argmax = rng.integers(0, S, COOKS_N).astype(np.int32)
    argmax[::7], argmax[3::7] = 0, S - 1
    menu = [cutoff, math.nextafter(cutoff, math.inf), math.nextafter(cutoff, 0.0), NAN, 0.5 * cutoff, 2.0 * cutoff, math.inf, 0.0]
    maxCooks = np.array([menu[i] for i in rng.integers(0, len(menu), COOKS_N)])
    maxCooks[:16] = np.tile([math.nextafter(cutoff, math.inf), 3.0 * cutoff], 8)   # flagged for certain, whatever the counts
    pvalue = rng.uniform(size=COOKS_N)
    pvalue[5::11] = NAN
    case = dict(name=name, group=group, counts=counts, argmax=argmax, maxCooks=maxCooks, pvalue=pvalue, cutoff=cutoff, p=p, m=m, applies=applies)
    _cooks_cache[name] = case
    return case


# ---------------------------------------------------------------------------------------------------------------------------
# IHW
# ---------------------------------------------------------------------------------------------------------------------------
def near_break(b, side):
    """a double d with log d within 1 ulp of the break b, below (side = -1: x <= b) or above it (side = +1: x > b); mpmath finds it"""
    import mpmath as mp
    with mp.workdps(rx.DPS):
        d = float(mp.exp(mp.mpf(b)))
        for _ in range(64):
            x = mp.log(mp.mpf(d))
            if (x > b) == (side > 0) and x != b:
                if abs(x - b) <= math.ulp(b):
                    return d
                raise AssertionError("no double within 1 ulp of the break on this side")
            d = math.nextafter(d, math.inf if side > 0 else 0.0)
    raise AssertionError("no double found")


IHW_CASES = ["ng1-inf", "ng2-finite", "ng7-inf", "ng7-dirty", "ng255-inf", "ng256-finite", "ng2-large"]
_ihw_cache = {}


def ihw_case(name):
    if name in _ihw_cache:
        return _ihw_cache[name]
    ng = int(name.split("-")[0][2:])
    rng = np.random.default_rng(3220 + ng + len(name))
    top = 16.0
    inner = np.sort(rng.uniform(1.0, top, ng - 1)) if ng > 1 else np.array([])
    breaks = np.concatenate([[0.0], inner, [math.inf if not name.endswith("finite") else top + 1.0]])
    w = rng.uniform(0.2, 3.0, ng)
    if ng >= 7:
        w[2] = 0.0                                   # p / 0
    if name == "ng2-large":
        n = 262145
        d = np.array([math.exp(0.5 * breaks[1]), -math.exp(0.5 * breaks[1]), math.exp(breaks[1] + 1.0), 1e9])
        av = d[rng.integers(0, 4, n)]
        w = np.array([1.5, 0.25])
        pv = rng.uniform(size=n)
        pv[::1001] = NAN
    else:
        n = 600
        av = np.exp(rng.uniform(0.01, top, n)) * rng.choice([-1.0, 1.0], n)
        pv = rng.uniform(size=n) ** 3
        pv[7::50] = NAN
        pv[9::50] = 0.0
        pos = 0
        # five rows at most: within the share of a case's rows that may be excused
        for b in breaks[1:-1][:2].tolist() + ([breaks[-1]] if math.isfinite(breaks[-1]) else []):
            for side in (-1, 1):
                if b == breaks[-1] and side > 0:
                    continue                          # beyond a finite last break: NA, the dirty case's
                av[pos] = near_break(b, side) * (-1.0 if pos % 2 else 1.0)
                pos += 1
        if math.isinf(breaks[-1]):
            av[pos], av[pos + 1] = math.inf, -math.inf   # log = +Inf: inside (b, Inf]
        if name.endswith("dirty"):
            av[-6:] = [0.0, NAN, 0.5, 1.0, -1.0, math.exp(-3.0)]   # log -Inf, NaN, below the first break, on it: NA groups
    case = dict(name=name, ng=ng, breaks=breaks, weights=w, avDist=np.ascontiguousarray(av), pvalue=np.ascontiguousarray(pv))
    _ihw_cache[name] = case
    return case


def chain_ihw_tables(rng=None):
    """seven made-up groups for the chained case"""
    return np.array([0.0, 8.0, 9.5, 10.5, 11.5, 12.5, 13.5, math.inf]), np.array([2.5, 2.0, 1.5, 1.0, 0.75, 0.5, 0.25])


def chain_avdist(n):
    return np.exp(np.random.default_rng(3232).uniform(7.0, 15.0, n))
