"""Inputs of tests/test_trend_twin.py and tests/test_gpu_trend.py: columns for the fit's global stage (baseMean, dispGeneEst, allZero,
S, p, options) with the edges of the mean trend, the local trend, the residual rules, the residual histogram and the simulated prior
planted; residual columns for the histogram kernel alone; three free fits.  Seeded and small: 599 rows unless a size is the point.

A stage case is dict(name, baseMean, dispGeneEst, allZero, S, p, opts = {fitType | trendCoef | dispPriorVar}, substitute (option
"local_trend_substitute"), error (the call must fail), note).  All-zero rows carry NaN in both columns, as the fit leaves them."""
import math

import numpy as np

MIN_DISP = 1e-8
T100, T10 = 100 * MIN_DISP, 10 * MIN_DISP  # the two thresholds, as the doubles the rules form
N = 599
PRIOR_V = (0.0, 0.1, 0.2, 0.3, 1.0, 4.0, 8.0, 12.0)
PRIOR_DESIGNS = {"S3p2": (3, 2), "S3~1": (3, 1), "S4-2v2": (4, 2), "S4~1": (4, 1), "S5-2v3": (5, 2)}  # d.f. 1, 2, 2, 3, 3
COEFS = (0.05, 2.0)  # the supplied trend of the prior cases


def _case(name, bm, al, S, p, opts, zero=None, substitute=1, error=False, note=""):
    bm, al = np.array(bm, dtype=np.float64), np.array(al, dtype=np.float64)
    az = np.zeros(len(bm), dtype=np.int32)
    if zero is not None:
        az[zero] = 1
        bm[zero] = np.nan
        al[zero] = np.nan
    return dict(name=name, baseMean=bm, dispGeneEst=al, allZero=az, S=S, p=p, opts=dict(opts), substitute=substitute, error=error, note=note)


def _near(v):
    return [np.nextafter(v, 0.0), v, np.nextafter(v, 1.0)]


def _trend_columns(rng, n, lo=1e-3, hi=1e9, sd=0.6):
    bm = np.exp(rng.uniform(math.log(lo), math.log(hi), n))
    al = np.exp(rng.normal(np.log(0.02 + 3.0 / np.sqrt(bm)), sd))
    return bm, np.clip(al, 2 * T100, 50.0)


def local_wide(S=8, p=2, seed=11, n=N):
    """Means over 1e-3 .. 1e9; duplicated means, several rows at the smallest and at the largest mean of the fit; ties of |x - xv| at
    rank k from both end vertices (five rows of one mean straddle the rank, so rows sit at |dx| = h exactly); rows at minDisp whose
    means lie below and above every mean of the fit (both continuations); dispGeneEst at 100 minDisp and at 10 minDisp with their
    neighbouring doubles; all-zero rows."""
    rng = np.random.default_rng(seed)
    nfit = 500
    bm, al = _trend_columns(rng, nfit)
    order = np.argsort(bm)
    bm, al = bm[order], al[order]
    k = int(math.floor(nfit * 0.7))
    bm[k - 2:k + 3] = bm[k]                      # from min x: ranks k - 1 .. k + 3 at one distance
    bm[nfit - k - 3:nfit - k + 2] = bm[nfit - k]  # from max x
    bm[:4] = bm[0]                               # several rows at the minimum ...
    bm[-3:] = bm[-1]                             # ... and at the maximum
    bm[100:103] = bm[100]
    bm[250] = bm[249]
    # rows outside the fit: at the floor, with means beyond both ends and inside; the boundary values of both rules
    out_bm = np.concatenate([bm[0] * np.array([0.5, 0.1, 1e-3]), bm[-1] * np.array([2.0, 10.0, 1e3]), rng.choice(bm, 40),
                             rng.choice(bm, 6), [bm[0], bm[-1]]])
    out_al = np.concatenate([np.full(46, MIN_DISP), _near(T100), _near(T10), [MIN_DISP, MIN_DISP]])
    nz = n - nfit - len(out_bm)
    bm = np.concatenate([bm, out_bm, np.ones(nz)])
    al = np.concatenate([al, out_al, np.ones(nz)])
    perm = rng.permutation(n)
    return _case(f"local-wide-S{S}p{p}", bm[perm], al[perm], S, p, dict(fitType=2), zero=np.flatnonzero(perm >= n - nz),
                 note="weights over twelve decades, ties at rank k, both continuations, threshold neighbours")


def local_sizes():
    rng = np.random.default_rng(12)
    out = []
    for n in (255, 256, 257):
        bm, al = _trend_columns(rng, n, 0.5, 1e5)
        out.append(_case(f"local-n{n}", bm, al, 8, 2, dict(fitType=2), zero=np.array([0, n - 1])))
    for nfit in (3, 4, 5):  # k = 2, 2, 3: too few rows; one row inside the bandwidth; two rows inside it (rank 2 of 3)
        bm = np.concatenate([np.array([2.0, 30.0, 400.0, 5e3, 6e4])[:nfit], [1.0, 1e6, 50.0]])
        al = np.concatenate([np.array([0.9, 0.5, 0.2, 0.1, 0.05])[:nfit], [MIN_DISP, MIN_DISP, T100]])
        out.append(_case(f"local-nfit{nfit}", bm, al, 8, 2, dict(fitType=2)))
    lx = 12.0 * np.random.default_rng(101).beta(3, 3, 300)  # means dense in the middle: a cell whose split score lies between 0.8 and 1
    bm = np.exp(lx)
    out.append(_case("local-dense-centre", bm, np.clip(np.exp(rng.normal(np.log(0.02 + 3.0 / np.sqrt(bm)), 0.6)), 2 * T100, 50.0), 8, 2, dict(fitType=2)))
    out.append(_case("local-n1", [7.0], [0.3], 8, 2, dict(fitType=2)))
    bm, al = _trend_columns(rng, 40, 1, 1e4)
    out.append(_case("local-equal-means", np.full(40, 123.456), al, 8, 2, dict(fitType=2)))
    bm, al = _trend_columns(rng, 100, 1, 1e4)
    bm[:72] = bm.min()  # >= 70 % of the rows at one mean that is also min x: h = 0 there
    out.append(_case("local-h0", bm, al, 8, 2, dict(fitType=2)))
    return out


def mean_cases():
    rng = np.random.default_rng(13)
    out = []
    for usable in (999, 1000, 1001, 1999, 2000):  # trim counts 0, 1, 1, 1, 2
        al = np.exp(rng.uniform(math.log(1e-6), math.log(1e6), usable))  # twelve orders of magnitude
        al[0], al[1] = 3e7, 2.5e-7           # what the trim takes away first
        al[2] = np.nextafter(T10, 1.0)       # the smallest usable value: the threshold's upper neighbour
        al = np.concatenate([al, _near(T10)[:2], np.full(5, MIN_DISP), [1.0, 1.0]])  # at and below the threshold: not usable; two all-zero rows
        bm = np.exp(rng.uniform(0, 10, len(al)))
        perm = rng.permutation(len(al))
        out.append(_case(f"mean-{usable}", bm[perm], al[perm], 8, 2, dict(fitType=1), zero=np.flatnonzero(perm >= len(al) - 2)))
    al = np.concatenate([np.full(20, MIN_DISP), _near(T10)[:2]])
    out.append(_case("mean-none-usable", np.exp(rng.uniform(0, 5, len(al))), al, 8, 2, dict(fitType=1), error=True))
    return out


def parametric_failures():
    """Columns on which the parametric trend fails: dispersions that RISE with the mean give a slope <= 0 in the first round."""
    rng = np.random.default_rng(14)
    bm = np.exp(rng.uniform(0.0, math.log(1e5), N))
    al = (0.5 - 0.4 / bm) * np.exp(rng.normal(0, 0.05, N))
    zero = np.array([5, 300])
    out = [_case("param-fails-coef-substituted", bm, al, 8, 2, dict(fitType=0), zero=zero),
           _case("param-fails-coef-reported", bm, al, 8, 2, dict(fitType=0), zero=zero, substitute=0)]
    # more than 10 rounds: a ladder of fourteen groups of rows, each 1.8 times further above the trend than the one before.  A round
    # takes in the group that the last round's coefficients brought below the filter's bound of 15, which raises the coefficients
    # enough to bring in the next: the coefficients stay positive and never settle.
    rng = np.random.default_rng(19)
    bm = np.exp(rng.uniform(0.0, math.log(1e4), N))
    al = (0.01 + 1.0 / bm) * np.exp(rng.normal(0, 0.1, N))
    idx, per, level = rng.permutation(N), int(0.05 * N), 12.0
    for j in range(14):
        al[idx[j * per:(j + 1) * per]] *= level
        level *= 1.8
    out.append(_case("param-fails-rounds-substituted", bm, al, 8, 2, dict(fitType=0), zero=np.array([7, 400])))
    return out


def draw_residuals(rng, df, v, n):
    return np.log(rng.chisquare(df, n) / df) + (rng.normal(0.0, math.sqrt(v), n) if v > 0 else 0.0)


def _prior_case(name, resid, S, p, rng, n=None, zero=None, note=""):
    """Columns whose residuals under the supplied trend COEFS are `resid` (up to the rounding of the product)."""
    n = len(resid) if n is None else n
    bm = np.exp(rng.uniform(0.0, 9.0, n))
    fit = COEFS[0] + COEFS[1] / bm
    al = np.maximum(fit * np.exp(resid), 2 * T100)
    return _case(name, bm, al, S, p, dict(trendCoef=COEFS), zero=zero, note=note)


def prior_cases():
    out = []
    for d, (S, p) in PRIOR_DESIGNS.items():
        for v in PRIOR_V:
            rng = np.random.default_rng(1000 * S + 100 * p + int(v * 10))
            out.append(_prior_case(f"prior-{d}-v{v:g}", draw_residuals(rng, S - p, v, N), S, p, rng, zero=np.array([0, 17, N - 1])))
    rng = np.random.default_rng(15)
    out.append(_prior_case("prior-df4-S6p2", draw_residuals(rng, 4, 0.3, N), 6, 2, rng, note="m - p = 4: the closed form"))
    out.append(_prior_case("prior-one-residual", np.array([0.37]), 4, 2, rng))
    out.append(_prior_case("prior-one-bin", rng.uniform(0.55, 0.95, N), 4, 2, rng))
    out.append(_prior_case("prior-extreme-bins", np.where(np.arange(N) % 2 == 0, -9.7, 9.7) + rng.uniform(-0.1, 0.1, N), 4, 2, rng))
    r = np.concatenate([draw_residuals(rng, 2, 4.0, 200), rng.uniform(10.5, 12.0, N - 200)])  # two thirds of the residuals outside (-10, 10)
    out.append(_prior_case("prior-many-outside", rng.permutation(r), 4, 2, rng))
    c = _prior_case("prior-none-inside", np.zeros(N), 4, 2, rng)
    c["dispGeneEst"] = np.where(np.arange(N) % 2 == 0, 1e-6, 1e-6 * (1 + 1e-9))  # log(1e-6 / dispFit) < -10 on every row
    c["baseMean"] = np.exp(rng.uniform(-3.0, 0.0, N))
    out.append(c)
    z = _case("all-rows-all-zero", np.ones(N), np.ones(N), 4, 2, dict(fitType=0), zero=np.arange(N))
    out.append(z)
    return out


def grid_wrap():
    """262 144 + 700 rows, all but about 600 all-zero, a few live rows beyond row 262 144: the 1 024 x 256-thread passes go round twice."""
    rng = np.random.default_rng(16)
    n = 262144 + 700
    live = np.sort(np.concatenate([rng.choice(262144, 560, replace=False), 262144 + rng.choice(700, 40, replace=False)]))
    bm, al = np.ones(n), np.ones(n)
    b, a = _trend_columns(rng, len(live), 1e-2, 1e7)
    bm[live], al[live] = b, a
    al[live[::50]] = MIN_DISP
    zero = np.setdiff1d(np.arange(n), live)
    return _case("grid-wrap-local-S4p2", bm, al, 4, 2, dict(fitType=2), zero=zero)


def stage_cases():
    return ([local_wide(8, 2), local_wide(4, 2, seed=21)] + local_sizes() + mean_cases() + parametric_failures() + prior_cases())


# ---- the histogram kernel alone -------------------------------------------------------------------------------------------
def hist_edge_values():
    """Every fuzzed break as the double brk + 5e-8 with its neighbours, brk itself with its neighbours, +-10 and their neighbours,
    +-Inf, NaN, +-0."""
    v = []
    for j in range(41):
        brk = j / 2.0 - 10.0
        for c in (brk, brk + 5e-8, brk - 5e-8):
            v += [np.nextafter(c, -np.inf), c, np.nextafter(c, np.inf)]
    v += [np.inf, -np.inf, np.nan, 0.0, -0.0, 11.0, -11.0, 1e300, -1e300, 5e-324, -5e-324]
    return np.array(v, dtype=np.float64)


HIST_SIZES = (65535, 65536, 65537, 2 * 65536 + 1)


def hist_column(n, seed=17):
    """n values: the edge values first and last, random residuals (some outside (-10, 10), some NaN) between."""
    rng = np.random.default_rng(seed + n)
    e = hist_edge_values()
    x = rng.normal(0.0, 4.5, n)
    x[rng.random(n) < 0.05] = np.nan
    x[:len(e)] = e
    x[-len(e):] = e[::-1]
    m = max(0, min(6, n - 65533))
    x[65533:65533 + m] = e[60:60 + m]  # edge values on both sides of row 65 536
    return x


# ---- free fits through the product path ---------------------------------------------------------------------------------
def free_fits():
    from chicdiff_amd import synth
    import test_gpu_parity as tgp
    a = synth.make(1500, 4)
    b = synth.make(1200, 8)
    counts, nf, group, _ = tgp._extreme_matrix()
    return {"S4-2v2": dict(counts=a["counts"], nf=a["nf"], group=a["group"], opts={}),
            "S8-local": dict(counts=b["counts"], nf=b["nf"], group=b["group"], opts=dict(fitType=2)),
            "extreme-substituted": dict(counts=counts, nf=nf, group=group, opts={})}
