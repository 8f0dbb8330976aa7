"""The trend's other branches and the simulated prior variance in 50-digit arithmetic (mpmath): fitType "mean", fitType "local" (also
DESeq2's substitute for a parametric trend that failed), the log residuals under any trend, the histogram of the residuals and
estimateDispersionsPriorVar for residual d.f. <= 3.

Written from the rule texts alone — include/chicdiff_hip.h (fitType, status bits), the heads of chicdiff_amd/csrc/prior_mc.h and
oracle/locfit_oracle.c, SURVEY.md Appendix A3 / A4 — and from R's documented definitions of mean(trim =), hist(right = TRUE) and
loess(surface = "interpolate"); not from the code under either head, not from the kernels.  It pins the arithmetic and the decisions
of those rules as this project states them; whether they are locfit's and R's is for tools/make_golden.R.

Reported doubles are exact inputs, as in tests/disp_twin.global_stage.  Every value is an mpf of DPS digits (callers work inside
`with mp.workdps(DPS)`) and comes with its UNIT, u = 2^-53 times the quantity's condition, derived from the inputs alone; every
discrete decision comes back with its margin and the unit of the values compared.  The units, with the count of roundings a
double-precision statement of the rule needs at the least (the a-priori bound of the yardstick in these units):

  mean trend          u mean (all terms positive: sum |terms| / count).  n - 2 lo additions and one division: n - 2 lo + 1 roundings of
                      relative size u in the worst order, 2 with a long-double accumulator.
  vertex x            u |x| at the two ends (one logarithm); a midpoint: the mean of its cell's two units + u (|x_l| + |x_r|) / 2.
  vertex h            u (|x_k| + |x_v|), x_k the row at rank k: one rounding each of the two logarithms, one of the difference: 3.
  vertex f, d         row 0 / row 1 of |M^-1| (E_T + E_S |b|): M the moment matrix S[j + k] in the basis 1, dx, dx^2, b its solution,
                      E_S[q], E_T[q] the sums over the rows of the first-order bounds of one term's error — the rounding of its own
                      log baseMean and of the vertex (u (|x_i| + |x_v|) in dx, through dx^q and through the kernel's argument), the
                      bandwidth's unit through the kernel's argument (dK/du u u_h / h), and (q + 4) u |term| for the products.  M^-1 is
                      adj(M) / det(M): the cancellation of the moments against the determinant is in it.  Roundings: 2 + (q + 4) per
                      term and 11 of the 3 x 3 solve.
  dispFit             exp(v) (|p0| u_f[j] + |p1| u_f[j+1] + z (|p2| u_d[j] + |p3| u_d[j+1]) + |dv/dx| u (|x| + |x_j| + |x_j+1|)
                      + 4 u sum |terms| + u): the vertices' units through the Hermite weights, the row's own logarithm, 8 roundings of
                      the polynomial and one of exp.
  residual            u (|log dispGeneEst| + |log dispFit|) + unit(dispFit) / dispFit: two logarithms, one difference.
  varLogDispEsts      tests/disp_twin.mad_stage on these residuals and units.
  KL sum              u sum_b obs_b (|log(obs_b + small)| + |log(dens_b + small)|): 40 terms of 5 roundings each.
  loess value         u sum_g |c_g(x) kl_g|, c the operator row of the fitted value at x (40 + 40 coefficients): 80 products, 79 additions.
"""
import math
from fractions import Fraction

import mpmath as mp

import disp_twin as dt

DPS = dt.DPS
U = mp.ldexp(mp.mpf(1), -53)
MIN_DISP = dt.MIN_DISP
MAX_VERTICES = 100  # locfit's maxk
NEAR_UNITS = 4      # a decision is "near" when its margin lies inside so many units of the values compared


class NoFit(Exception):
    """The rule gives no local fit: fewer than four rows, max x = min x, h = 0, a singular system."""


def _f(v):
    return mp.mpf(float(v))


def live_rows(baseMean, dispGeneEst, allZero=None):
    return [i for i in range(len(baseMean))
            if (allZero is None or not int(allZero[i])) and baseMean[i] == baseMean[i] and dispGeneEst[i] == dispGeneEst[i]]


# ---------------------------------------------------------------------------------------------------------------------------
# fitType "mean": mean(dispGeneEst[dispGeneEst > 10 minDisp], trim = 0.001)
# ---------------------------------------------------------------------------------------------------------------------------
def mean_trend(dispGeneEst, allZero=None, min_disp=MIN_DISP, factor=10, trim=0.001, count=math.floor):
    """R's mean(x, trim): lo = floor(n trim) (the product in double arithmetic, as R forms it), the mean of elements lo + 1 .. n - lo
    of the sorted vector, as an exact rational.  Returns dict(failed, value, unit, n, lo, near = (margin, unit) of the element closest
    to the threshold).  `factor`, `trim`, `count`: the wrong readings of tests/test_trend_twin.py."""
    thr = factor * min_disp  # (a double product, in R as here)
    vals = [float(v) for i, v in enumerate(dispGeneEst) if v == v and (allZero is None or not int(allZero[i]))]
    use = sorted(v for v in vals if v > thr)
    near = min(((abs(_f(v) - _f(thr)), U * _f(thr)) for v in vals), default=(mp.inf, U), key=lambda t: t[0])
    n = len(use)
    if n == 0:
        return dict(failed=True, n=0, lo=0, near=near)
    lo = int(count(n * trim))
    kept = use[lo:n - lo]
    value = sum(Fraction(v) for v in kept) / len(kept)
    value = mp.mpf(value.numerator) / mp.mpf(value.denominator)
    return dict(failed=False, value=value, unit=U * value, n=n, lo=lo, near=near)


# ---------------------------------------------------------------------------------------------------------------------------
# fitType "local": locfit(log disp ~ log mean, weights = mean), alpha = 0.7, deg = 2, tricube, rbox(cut = 0.8), Hermite
# ---------------------------------------------------------------------------------------------------------------------------
def _kernel(u, kind):
    """(K(u), dK/du) for 0 <= u < 1."""
    if kind == "tricube":
        c = 1 - u ** 3
        return c ** 3, 9 * u * u * c * c
    c = 1 - u * u  # bisquare: a wrong reading
    return c * c, 4 * u * c


def local_trend(baseMean, dispGeneEst, allZero=None, min_disp=MIN_DISP, strict=True, kfun=math.floor, weights=True, kernel="tricube",
                cut=0.8, linear_outside=True, scale_slopes=True, flip=()):
    """The local trend on reported columns.  Rows in the fit: dispGeneEst > 100 minDisp; x = log baseMean; k = floor(0.7 nfit) (the
    product in double arithmetic, as locfit forms it); h(xv) = the k-th smallest |x - xv|; tricube weights times baseMean; local
    quadratic in the basis 1, dx, dx^2 / 2, value and slope at xv by an exact solve; vertices min x and max x, then a cell cut at its
    midpoint while length / min(h_l, h_r) > 0.8; cubic Hermite inside a cell, the end vertex's line outside [min x, max x].

    Returns dict(failed = None | reason, nfit, k, vertices = [dict(x, h, f, d, u_x, u_h, u_f, u_d)] ascending, decisions = [dict(kind
    "split", margin, unit, cell)], dispFit / log_fit / unit / unit_log / cls / edge per row given (None for rows without counts): cls in
    "interior", "left", "right", "vertex"; edge = (distance to the nearest inner vertex, unit)).  flip: indices into `decisions` taken
    the other way.  The other keywords are the wrong readings of tests/test_trend_twin.py."""
    thr = _f(100 * min_disp)
    rows = live_rows(baseMean, dispGeneEst, allZero)
    bm = {i: _f(baseMean[i]) for i in rows}
    al = {i: _f(dispGeneEst[i]) for i in rows}
    fit = [i for i in rows if (al[i] > thr if strict else al[i] >= thr)]
    n = len(baseMean)
    res = dict(failed=None, nfit=len(fit), k=None, vertices=[], decisions=[], dispFit=[None] * n, log_fit=[None] * n, unit=[None] * n,
               unit_log=[None] * n, cls=[None] * n, edge=[None] * n)
    try:
        if len(fit) < 4:
            raise NoFit("fewer than four rows")
        x = {i: mp.log(bm[i]) for i in rows}
        y = {i: mp.log(al[i]) for i in fit}
        lo, hi = min(x[i] for i in fit), max(x[i] for i in fit)
        if not hi > lo:
            raise NoFit("max x = min x")
        k = int(kfun(len(fit) * 0.7))
        res["k"] = k
        if k < 1:
            raise NoFit("k < 1")
        verts = []

        def vertex(xv, u_x=None):
            if len(verts) >= MAX_VERTICES:
                raise NoFit("more than 100 vertices")
            dist = sorted((abs(x[i] - xv), i) for i in fit)
            h, ik = dist[min(k, len(dist)) - 1]
            if not h > 0:
                raise NoFit("h = 0")
            u_h = U * (abs(x[ik]) + abs(xv))
            S, T, ES, ET = [mp.mpf(0)] * 5, [mp.mpf(0)] * 3, [mp.mpf(0)] * 5, [mp.mpf(0)] * 3
            for d_, i in dist:
                if d_ >= h:
                    break
                dx, uu = x[i] - xv, d_ / h
                K, dK = _kernel(uu, kernel)
                wg = bm[i] if weights else mp.mpf(1)
                w = wg * K
                u_dx = U * (abs(x[i]) + abs(xv))
                e_w = wg * dK * (u_dx / h + uu * u_h / h)
                for q in range(5):
                    term = w * dx ** q
                    e = abs(dx) ** q * e_w + (q * w * abs(dx) ** (q - 1) * u_dx if q else 0) + (q + 4) * U * abs(term)
                    S[q], ES[q] = S[q] + term, ES[q] + e
                    if q < 3:
                        T[q], ET[q] = T[q] + term * y[i], ET[q] + e * abs(y[i]) + 2 * U * abs(term * y[i])
            M = mp.matrix(3, 3)
            for j in range(3):
                for q in range(3):
                    M[j, q] = S[j + q]
            det = mp.det(M)
            scale = S[0] * S[2] * S[4]
            if det == 0 or scale == 0 or abs(det) < mp.mpf(10) ** (-(DPS - 10)) * abs(scale):
                raise NoFit("singular system")
            Mi = M ** -1
            b = Mi * mp.matrix(T)
            cond = [mp.fsum(abs(Mi[r, j]) * (ET[j] + mp.fsum(ES[j + q] * abs(b[q]) for q in range(3))) for j in range(3)) for r in (0, 1)]
            verts.append(dict(x=xv, h=h, f=b[0], d=b[1], u_x=U * abs(xv) if u_x is None else u_x, u_h=u_h, u_f=cond[0] + U * abs(b[0]), u_d=cond[1] + U * abs(b[1])))
            return len(verts) - 1

        def grow(il, ir):
            l, r = verts[il], verts[ir]
            le = r["x"] - l["x"]
            hm = l if l["h"] <= r["h"] else r
            margin = le - mp.mpf(cut) * hm["h"]
            res["decisions"].append(dict(kind="split", margin=margin, unit=U * (abs(l["x"]) + abs(r["x"])) + mp.mpf(cut) * hm["u_h"],
                                         cell=(l["x"], r["x"])))
            ans = margin > 0
            if len(res["decisions"]) - 1 in flip:
                ans = not ans
            if not ans:
                return
            im = vertex((l["x"] + r["x"]) / 2, (l["u_x"] + r["u_x"]) / 2 + U * (abs(l["x"]) + abs(r["x"])) / 2)
            grow(il, im)
            grow(im, ir)

        il = vertex(lo)
        ir = vertex(hi)
        grow(il, ir)
    except NoFit as e:
        res["failed"] = str(e)
        return res
    verts.sort(key=lambda v: v["x"])
    res["vertices"] = verts
    nv = len(verts)
    for i in rows:
        xr = x[i]
        j = 0
        while j + 2 < nv and xr >= verts[j + 1]["x"]:
            j += 1
        a, b_ = verts[j], verts[j + 1]
        z = b_["x"] - a["x"]
        t = (xr - a["x"]) / z
        sl = z if scale_slopes else mp.mpf(1)
        if t < 0:
            p, dp, cls = (1, 0, t if linear_outside else 0, 0), (0, 0, 1 if linear_outside else 0, 0), "left"
        elif t > 1:
            p, dp, cls = (0, 1, 0, (t - 1) if linear_outside else 0), (0, 0, 0, 1 if linear_outside else 0), "right"
        else:
            p1 = t * t * (3 - 2 * t)
            p = (1 - p1, p1, t * (1 - t) ** 2, t * t * (t - 1))
            dp = (-6 * t * (1 - t), 6 * t * (1 - t), (1 - t) * (1 - 3 * t), t * (3 * t - 2))
            cls = "vertex" if any(xr == v["x"] for v in verts) else "interior"
        terms = (p[0] * a["f"], p[1] * b_["f"], p[2] * a["d"] * sl, p[3] * b_["d"] * sl)
        v = mp.fsum(terms)
        dvdx = (dp[0] * a["f"] + dp[1] * b_["f"]) / z + (dp[2] * a["d"] + dp[3] * b_["d"]) * sl / z
        u_log = (abs(p[0]) * a["u_f"] + abs(p[1]) * b_["u_f"] + z * (abs(p[2]) * a["u_d"] + abs(p[3]) * b_["u_d"])
                 + abs(dvdx) * U * (abs(xr) + abs(a["x"]) + abs(b_["x"])) + 4 * U * mp.fsum(abs(s) for s in terms))
        fitv = mp.exp(v)
        res["log_fit"][i], res["dispFit"][i], res["unit_log"][i], res["unit"][i], res["cls"][i] = v, fitv, u_log, fitv * (u_log + U), cls
        inner = [(abs(xr - w["x"]), U * (abs(xr) + abs(w["x"]))) for w in verts[1:-1] if xr != w["x"]]
        res["edge"][i] = min(inner, key=lambda e: e[0] / e[1]) if inner else None
    return res


# ---------------------------------------------------------------------------------------------------------------------------
# residuals, their histogram
# ---------------------------------------------------------------------------------------------------------------------------
def residuals(dispGeneEst, dispFit, unit_fit, allZero=None, min_disp=MIN_DISP, strict=False):
    """log dispGeneEst - log dispFit over dispGeneEst >= 100 minDisp.  dispFit, unit_fit: per row (mpf or None), under any trend.
    Returns (values, units): lists with None where the row has no residual."""
    thr = _f(100 * min_disp)
    n = len(dispGeneEst)
    val, unit = [None] * n, [None] * n
    for i in range(n):
        g = dispGeneEst[i]
        if g != g or dispFit[i] is None or (allZero is not None and int(allZero[i])):
            continue
        g = _f(g)
        if not (g > thr if strict else g >= thr):
            continue
        lg, lf = mp.log(g), mp.log(dispFit[i])
        val[i], unit[i] = lg - lf, U * (abs(lg) + abs(lf)) + unit_fit[i] / dispFit[i]
    return val, unit


FUZZ = 5e-8  # 1e-7 * median(diff(-20:20/2)), as a double


def fuzzed_breaks(fuzz=FUZZ):
    """hist.default's breaks for -20:20/2: every break moved up by the double `fuzz` (a double sum), the first one down."""
    b = [j / 2.0 - 10.0 for j in range(41)]
    return [b[0] - fuzz] + [v + fuzz for v in b[1:]]


def resid_hist(values, units=None, right=True, fuzz=FUZZ):
    """hist(x[x > -10 & x < 10], breaks = -20:20/2)$counts on exact values (doubles or mpf; None / NaN = no residual): bin j holds
    fb_j < x <= fb_j+1.  Returns (counts[40], info = [(index, bin, distance to the nearest fuzzed break or +-10, unit)])."""
    if units is None and not any(isinstance(v, mp.mpf) for v in values):
        # doubles against doubles: the comparisons are exact as they stand (the distances are not worked out)
        import bisect
        fbd, counts = fuzzed_breaks(fuzz), [0] * 40
        for v in values:
            if v is not None and v == v and -10.0 < v < 10.0:
                counts[(bisect.bisect_left(fbd, v) if right else bisect.bisect_right(fbd, v)) - 1] += 1
        return counts, []
    fb = [_f(v) for v in fuzzed_breaks(fuzz)]
    counts, info = [0] * 40, []
    for i, v in enumerate(values):
        if v is None or v != v:
            continue
        xv = v if isinstance(v, mp.mpf) else _f(v)
        if not (xv > -10 and xv < 10):
            info.append((i, -1, min(abs(xv + 10), abs(xv - 10)), units[i] if units else mp.mpf(0)))
            continue
        if right:
            j = max(q for q in range(40) if fb[q] < xv)
        else:
            j = max(q for q in range(40) if fb[q] <= xv)
        counts[j] += 1
        info.append((i, j, min([abs(xv - e) for e in fb] + [abs(xv + 10), abs(xv - 10)]), units[i] if units else mp.mpf(0)))
    return counts, info


# ---------------------------------------------------------------------------------------------------------------------------
# estimateDispersionsPriorVar, m - p <= 3
# ---------------------------------------------------------------------------------------------------------------------------
GRID, FINE, NEAR_Q, LEAF = 200, 1000, 40, 8
_OPERATORS = {}


def grid_x(g, n=GRID):
    return mp.mpf(8 * g) / (n - 1)  # seq(0, 8, length = n)


def loess_vertices():
    """Vertices of the k-d tree over the 200 grid values: the box widened by 0.5 % of its width, leaves of at most 8 points, a cell cut
    between its two middle points."""
    margin = mp.mpf(8) * mp.mpf("0.005")
    out = [-margin, 8 + margin]

    def split(l, u):  # 1-based, inclusive
        if u - l + 1 <= LEAF:
            return
        m = (l + u) // 2
        out.append((grid_x(m - 1) + grid_x(m)) / 2)
        split(l, m)
        split(m + 1, u)
    split(1, GRID)
    return sorted(out)


def loess_operator(span=0.2, degree=2):
    """Per vertex: (position, first grid index, coefficients of the value, coefficients of the slope) of the local fit over the q =
    floor(200 span) nearest grid values, tricube weights with h = the distance of the q-th nearest, solved exactly."""
    key = (span, degree)
    if key in _OPERATORS:
        return _OPERATORS[key]
    q = int(math.floor(GRID * span + 1e-5))
    xs = [grid_x(g) for g in range(GRID)]
    ops = []
    for s in loess_vertices():
        near = sorted(range(GRID), key=lambda g: (abs(xs[g] - s), g))[:q]
        lo = min(near)
        assert sorted(near) == list(range(lo, lo + q))
        h = max(abs(xs[g] - s) for g in near)
        w = [(1 - (abs(xs[g] - s) / h) ** 3) ** 3 for g in range(lo, lo + q)]
        dx = [xs[g] - s for g in range(lo, lo + q)]
        m = degree + 1
        M = mp.matrix(m, m)
        for a in range(m):
            for b in range(m):
                M[a, b] = mp.fsum(wi * d ** (a + b) for wi, d in zip(w, dx))
        Mi = M ** -1
        val = [wi * mp.fsum(Mi[0, a] * d ** a for a in range(m)) for wi, d in zip(w, dx)]
        slope = [wi * mp.fsum(Mi[1, a] * d ** a for a in range(m)) for wi, d in zip(w, dx)]
        ops.append((s, lo, val, slope))
    _OPERATORS[key] = ops
    return ops


def loess_rows(span=0.2, degree=2):
    """For each of the 1 000 fine values: the operator row {grid index: coefficient} of predict(lofit, x) — cubic Hermite blending of
    the two vertices around x."""
    key = ("rows", span, degree)
    if key in _OPERATORS:
        return _OPERATORS[key]
    ops = loess_operator(span, degree)
    rows = []
    for f in range(FINE):
        xf = grid_x(f, FINE)
        c = 0
        while c < len(ops) - 2 and xf > ops[c + 1][0]:
            c += 1
        (s0, l0, v0, d0), (s1, l1, v1, d1) = ops[c], ops[c + 1]
        wdt = s1 - s0
        t = (xf - s0) / wdt
        phi0, phi1 = (1 - t) ** 2 * (1 + 2 * t), t * t * (3 - 2 * t)
        psi0, psi1 = t * (1 - t) ** 2 * wdt, -t * t * (1 - t) * wdt
        row = {}
        for j in range(len(v0)):
            row[l0 + j] = row.get(l0 + j, 0) + phi0 * v0[j] + psi0 * d0[j]
            row[l1 + j] = row.get(l1 + j, 0) + phi1 * v1[j] + psi1 * d1[j]
        rows.append(row)
    _OPERATORS[key] = rows
    return rows


def kl_sums(hist, dens, all_count=None, small_from="both", exchanged=False):
    """The 200 KL sums of the observed density (counts / (0.5 sum counts)) from the simulated ones.  Returns [(kl, T)], T = the sum of
    the absolute values of the terms.  all_count / small_from / exchanged: wrong readings."""
    tot = sum(int(c) for c in hist) if all_count is None else all_count
    obs = [mp.mpf(2 * int(c)) / tot for c in hist]
    out = []
    for g in range(GRID):
        dg = [_f(v) for v in dens[g]]
        pos = [v for v in obs if v > 0] + ([v for v in dg if v > 0] if small_from == "both" else [])
        small = min(pos)
        a, b = (dg, obs) if exchanged else (obs, dg)
        la, lb = [mp.log(v + small) for v in a], [mp.log(v + small) for v in b]
        out.append((mp.fsum(v * (p - r) for v, p, r in zip(a, la, lb)), mp.fsum(v * (abs(p) + abs(r)) for v, p, r in zip(a, la, lb))))
    return out


def loess_fitted(kl, span=0.2, degree=2):
    """predict(loess(kl ~ x, span, degree), seq(0, 8, length = 1000)) and the unit of each value; kl: 200 mpf (or doubles, taken as exact)."""
    kl = [v if isinstance(v, mp.mpf) else _f(v) for v in kl]
    rows = loess_rows(span, degree)
    return ([mp.fsum(c * kl[g] for g, c in r.items()) for r in rows], [U * mp.fsum(abs(c * kl[g]) for g, c in r.items()) for r in rows])


def prior_var_mc(hist, dens, m_minus_p, var_log_disp_ests=None, span=0.2, degree=2, first=True, floor=True, **kl_kw):
    """estimateDispersionsPriorVar for m - p <= 3 from the 40 counts of the residuals inside (-10, 10) and the 200 x 40 simulated
    densities.  No residual inside: the closed form max(varLogDispEsts - trigamma((m - p) / 2), 0.25).  Returns dict(value, argmin,
    runner_up, gap = (difference of the two fitted values, sum of their units), kl, kl_unit, fitted, fitted_unit, closed_form)."""
    if sum(int(c) for c in hist) == 0:
        v = mp.mpf(var_log_disp_ests) - mp.polygamma(1, mp.mpf(m_minus_p) / 2)
        return dict(value=v if v > mp.mpf(0.25) else mp.mpf(0.25), closed_form=True, argmin=None)
    ks = kl_sums(hist, dens, **kl_kw)
    kl = [a for a, _ in ks]
    fitted, unit = loess_fitted(kl, span, degree)
    best = min(fitted)
    idx = [f for f in range(FINE) if fitted[f] == best]
    arg = idx[0] if first else idx[-1]
    others = [f for f in range(FINE) if f != arg]
    ru = min(others, key=lambda f: (fitted[f], f))
    x = grid_x(arg, FINE)
    value = x if (x > mp.mpf(0.25) or not floor) else mp.mpf(0.25)
    return dict(value=value, argmin=arg, runner_up=ru, gap=(fitted[ru] - fitted[arg], unit[ru] + unit[arg]), kl=kl, kl_unit=[U * t for _, t in ks],
                fitted=fitted, fitted_unit=unit, closed_form=False)


def by_simulation(S, p, prior_given=False, limit=3):
    """The prior variance is found by simulation: m - p <= 3 and none supplied."""
    return (not prior_given) and 0 < S - p <= limit


_DENS = {}


def simulated_densities(df):
    """The 200 x 40 simulated densities of residual d.f. `df` from the library's host entry (tests/test_r_rng.py holds them bit for
    bit to the oracle's): an input of the twin, not restated here."""
    if df not in _DENS:
        import numpy as np

        from chicdiff_amd import hip
        out = np.empty((200, 40))
        assert hip.load_library().chicdiff_hip_selftest_prior_mc(int(df), None, out.ctypes.data, None) == 0
        _DENS[df] = out
    return _DENS[df]
