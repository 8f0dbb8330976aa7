"""The results stage — pvalue -> padj, weight, weighted_padj — in exact rationals (fractions.Fraction) wherever the operation is
rational and in 50-digit arithmetic (mpmath) for lowess, the square root, log and qf.

Written from SURVEY.md Appendix A6, chicdiff.R:2038-2049 and R's documented definitions of quantile(type = 7), seq(length.out =),
p.adjust("BH"), cut() and lowess (Cleveland 1979, as stats::lowess documents it: f the smoother span, iter robustifying iterations
with bisquare weights on residuals scaled by 6 median |residual|, delta the distance inside which fits are interpolated) — not from
tests/results_twin.py, not from post_kernels.hip and not from the oracle, and it shares no code with any of them.

Two kinds of answer.  A VALUE comes with its unit (u = 2^-53 times the quantity's condition with respect to the roundings a double
evaluation must make); a DECISION comes with its margin — how far, in units, its two sides are apart.  Where R itself decides on
rounded doubles (BH: fl(fl(m / r) p) < alpha; filter >= cut) the IEEE sequence IS the requirement and plain Python floats execute it;
the exact rational value of the same comparison is reported beside it, and how often the two disagree is a statistic of the inputs.

UNITS
  theta_k     lower + k (upper - lower) / 49, three roundings: unit = u (|lower| + 2 |theta_k|).
  cut_f       type 7: x_(j) + g (x_(j+1) - x_(j)), h = (n - 1) theta = j + g.  A double h is off by up to (n - 1) unit(theta) + u h, which
              moves the cut along the segment; charged to the inputs as the earlier twins charge cancellation:
                  unit(cut) = u (|cut| + h |x_(j+1) - x_(j)|)     (where h is within 4 ulp of an integer t, the larger of the two
              segments that meet at x_(t): a double h may land on either).
              The BAND of a cut is the set of baseMean values within 4 units of it: whether such a row passes `filter >= cut` is a
              rounding matter; every other row passes or fails whatever the roundings.
  lowess      fit_i = sum_j l_j y_j; the weights take x_j - xs and x_j - a (cancellation: u max|x| absolute against a window of half
              width h_i) and the sum itself:  base_i = u (1 + max|x| / h_i) max|y|.  A robustness iteration reads weights off the
              residuals of the one before: an error e in a residual moves a bisquare weight by at most 1.54 e / cmad and cmad by 6 e,
              so  unit_t,i = base_i + 11 (max|res| / cmad_t) max_i unit_(t-1),i.
              Where cmad_t itself is within NOISE units of zero (a profile the smoother reproduces: constant, or a line) a double
              evaluation reads its bisquare weights off residuals that are rounding noise: they come out anywhere in [0, 1], the
              local regressions that follow are as ill-conditioned as those weights make them, and no unit bounds the result.  R is
              in the same position.  `ill` reports it — the weights were taken from such residuals, or the smoother stopped
              only because of a comparison (cmad < 1e-7 mean|res|) that is noise on both sides; a cmad of exactly 0 beside residuals
              well above the units (a step: most points are reproduced exactly) stops every evaluation and is not ill —; the fitted
              values are then no requirement (the index still is).
  thresh      max(fit) - sqrt(mean(residual^2)): unit = 2 max_i unit(fit_i).
  weight      avWeights_g / mean: the mean's n - 1 additions of positive terms and two divisions: unit = u weight (n + 1) — any order
              of summation is within it; weighted_pvalue = p / weight, one more rounding, judged against the weight it was given.
"""
import math
from fractions import Fraction

import mpmath as mp

DPS = 50
U = Fraction(1, 2 ** 53)
NQ = 50          # theta <- seq(lower, upper, length = 50)
BAND = 4         # units either side of a cut
NEAR_INT = 4     # ulps of h
NOISE = 64       # units: a 6-median-residual below this is rounding noise in double arithmetic
NA_INT = -2 ** 31


def ulp(x):
    return math.ulp(float(x))


# ---------------------------------------------------------------------------------------------------------------------------
# Cook's filter
# ---------------------------------------------------------------------------------------------------------------------------
_QF = {}


def qf99(d1, d2):
    """qf(.99, d1, d2) at 50 digits: the root of I_{d1 x / (d1 x + d2)}(d1 / 2, d2 / 2) = .99 by bisection (the F distribution's
    cdf is the regularised incomplete beta function)."""
    if (d1, d2) not in _QF:
        with mp.workdps(DPS + 10):
            target = mp.mpf(99) / 100
            cdf = lambda x: mp.betainc(mp.mpf(d1) / 2, mp.mpf(d2) / 2, 0, d1 * x / (d1 * x + d2), regularized=True)
            lo, hi = mp.mpf(0), mp.mpf(1)
            while cdf(hi) < target:
                hi *= 2
            for _ in range(4 * DPS):
                mid = (lo + hi) / 2
                if cdf(mid) < target:
                    lo = mid
                else:
                    hi = mid
            _QF[(d1, d2)] = (lo + hi) / 2
    return _QF[(d1, d2)]


def ulps_from_qf(value, d1, d2):
    """how far a double (scipy.stats.f.ppf's, say) is from the exact quantile, in ulps of the quantile"""
    with mp.workdps(DPS):
        q = qf99(d1, d2)
        return float(abs(mp.mpf(float(value)) - q) / ulp(q))


def design(group):
    """(m, p, applies): p = 1 for ~1 (one level), 2 for ~condition; the cutoff applies when m > p and some group has >= 3 samples"""
    g = [int(v) for v in group]
    m, levels = len(g), sorted(set(g))
    p = len(levels)
    return m, p, m > p and max(g.count(l) for l in levels) >= 3


def cooks_filter(counts, group, maxCooks, argmax, pvalue, cutoff):
    """counts: n rows of S ints.  Returns dict(applies, p (floats, NaN = NA), outlier (bools), larger (None or the number of counts
    strictly above the flagged sample's)).  Every comparison is between doubles or ints: there are no margins, only edges."""
    m, p, applies = design(group)
    out = [float(v) for v in pvalue]
    flags, larger = [False] * len(out), [None] * len(out)
    if applies:
        for i, mc in enumerate(maxCooks):
            mc = float(mc)
            if math.isnan(mc) or not mc > float(cutoff):
                continue
            flag = True
            if p == 2:
                row = [int(v) for v in counts[i]]
                larger[i] = sum(1 for v in row if v > row[int(argmax[i])])
                flag = larger[i] < 3
            if flag:
                flags[i], out[i] = True, math.nan
    return dict(applies=applies, p=out, outlier=flags, larger=larger)


# ---------------------------------------------------------------------------------------------------------------------------
# independent filtering: theta, cuts
# ---------------------------------------------------------------------------------------------------------------------------
def cuts(baseMean):
    """Exact lower, upper, theta, h and type-7 cuts of a finite baseMean.  Returns a dict of lists over the 50 quantiles:
    theta, h (Fractions), near_int (h within NEAR_INT ulp of an integer), cut (Fraction), unit (Fraction), band (the distinct
    baseMean values within BAND units of the cut), theta_unit."""
    x = sorted(Fraction(float(v)) for v in baseMean)
    n = len(x)
    lower = Fraction(sum(1 for v in x if v == 0), n)
    upper = Fraction(95, 100) if lower < Fraction(95, 100) else Fraction(1)
    distinct = sorted(set(x))
    res = dict(lower=lower, upper=upper, n=n, theta=[], theta_unit=[], h=[], near_int=[], cut=[], unit=[], band=[])
    for k in range(NQ):
        th = lower + k * (upper - lower) / (NQ - 1)
        h = (n - 1) * th
        j = h.numerator // h.denominator
        g = h - j
        nearest = round(h)
        near = abs(h - nearest) <= NEAR_INT * Fraction(ulp(max(float(h), 1.0)))
        xlo, xhi = x[j], x[min(j + 1, n - 1)]
        cut = xlo + g * (xhi - xlo)
        t = min(int(nearest), n - 1)
        seg = max(abs(x[min(t + 1, n - 1)] - x[t]), abs(x[t] - x[max(t - 1, 0)])) if near else abs(xhi - xlo)
        unit = U * (abs(cut) + h * seg) if seg else Fraction(0)   # equal neighbours: quantile() copies the value, whatever h's rounding
        res["theta"].append(th); res["theta_unit"].append(U * (lower + 2 * th)); res["h"].append(h); res["near_int"].append(near)
        res["cut"].append(cut); res["unit"].append(unit)
        res["band"].append([v for v in distinct if abs(v - cut) <= BAND * unit] if unit else [])
    return res


# ---------------------------------------------------------------------------------------------------------------------------
# BH: the IEEE sequence and the exact one
# ---------------------------------------------------------------------------------------------------------------------------
def bh_ieee(p):
    """p.adjust(p, "BH") as R executes it on doubles: n = number of non-NA; by decreasing p, cummin(fl(fl(n / i) p_(i))), pmin(1, .);
    NA stays NA.  Python floats are IEEE doubles: this IS the sequence."""
    idx = [i for i, v in enumerate(p) if not math.isnan(v)]
    n = len(idx)
    out = [math.nan] * len(p)
    order = sorted(idx, key=lambda i: p[i])
    run = math.inf
    for r in range(n, 0, -1):
        i = order[r - 1]
        run = min(run, (n / r) * p[i])
        out[i] = min(1.0, run)
    return out


def _below(m, r, p, a, A, ieee):
    """m / r * p < alpha: on doubles, or exactly (the rationals are formed only where the doubles are within 1e-12 of the edge)"""
    v = (m / r) * p
    if ieee or abs(v - a) > 1e-12 * a:
        return v < a
    return Fraction(m, r) * Fraction(p) < A


def num_rej(ps, alpha, ieee=True):
    """ps: the ascending non-NA p-values of the rows that pass.  The number with padj < alpha = the largest rank r with
    m / r * p_(r) < alpha (padj is a suffix minimum, so every rank below qualifies with it).  ieee: fl(fl(m / r) p) < alpha on
    doubles; otherwise the exact rational m p / r < alpha."""
    m, a, A = len(ps), float(alpha), Fraction(float(alpha))
    for r in range(m, 0, -1):
        if _below(m, r, ps[r - 1], a, A, ieee):
            return r
    return 0


def edge_disagreements(ps, alpha):
    """ranks on which the IEEE and the exact comparison fall on different sides of alpha"""
    m, a, A = len(ps), float(alpha), Fraction(float(alpha))
    return sum(1 for r in range(1, m + 1) if _below(m, r, ps[r - 1], a, A, True) != _below(m, r, ps[r - 1], a, A, False))


def pass_sets(baseMean, c, f, gt=False):
    """the readings of `filter >= cut_f` as boolean lists over the rows: [rows of the band fail, rows of the band pass], one entry
    where the band is empty (then rounding decides nothing).  gt: `>` in place of `>=` (a wrong reading, for the tests)."""
    distinct = sorted(set(Fraction(float(v)) for v in baseMean))
    rank = {float(v): i for i, v in enumerate(distinct)}
    cut, band = c["cut"][f], {rank[float(v)] for v in c["band"][f]}
    first = next((i for i, v in enumerate(distinct) if (v > cut if gt else v >= cut)), len(distinct))
    rows = [rank[float(v)] for v in baseMean]
    if not band:
        return [[r >= first for r in rows]]
    return [[r >= first and r not in band for r in rows], [r >= first or r in band for r in rows]]


def num_rej_readings(baseMean, pvalue, alpha, c):
    """c = cuts(baseMean).  Per filter: dict(ieee = the readings' IEEE counts [band rows fail, band rows pass] (one entry when the
    band is empty), exact = the same in rationals, disagree = ranks where IEEE and exact differ (last reading), m = rows counted)."""
    order = sorted((i for i, p in enumerate(pvalue) if not math.isnan(p)), key=lambda i: float(pvalue[i]))
    out = []
    for f in range(NQ):
        sets = [[float(pvalue[i]) for i in order if s[i]] for s in pass_sets(baseMean, c, f)]
        out.append(dict(ieee=[num_rej(s, alpha) for s in sets], exact=[num_rej(s, alpha, ieee=False) for s in sets],
                        disagree=edge_disagreements(sets[-1], alpha), m=[len(s) for s in sets]))
    return out


# ---------------------------------------------------------------------------------------------------------------------------
# lowess at 50 digits, every comparison with its margin
# ---------------------------------------------------------------------------------------------------------------------------
class Decisions(list):
    def take(self, name, lhs, rhs, scale, op):
        """records |lhs - rhs| / scale (inf for scale 0 and lhs != rhs; 0 for a tie) and returns lhs op rhs"""
        d = abs(lhs - rhs)
        self.append((name, math.inf if (scale == 0 and d != 0) else 0.0 if d == 0 else float(d / scale)))
        return op(lhs, rhs)


def lowess(x, y, f=Fraction(1, 5), iters=3, decisions=None):
    """x: ascending Fractions; y: numbers.  Returns (fit (mpf), unit (mpf), decisions); decisions.ill: see UNITS.  delta = 0.01
    range(x)."""
    dec = Decisions() if decisions is None else decisions
    gt, le, lt = (lambda a, b: a > b), (lambda a, b: a <= b), (lambda a, b: a < b)
    with mp.workdps(DPS):
        u = mp.mpf(1) / 2 ** 53
        n = len(x)
        xs = [mp.mpf(v.numerator) / v.denominator for v in x]
        ys = [mp.mpf(v) for v in y]
        rng = xs[-1] - xs[0]
        delta = rng / 100
        xmax, ymax = max(abs(v) for v in xs), max(abs(v) for v in ys)
        ns = max(2, min(n, int(f * n + Fraction(1, 10 ** 7))))
        rw = [mp.mpf(1)] * n
        fit, unit = [mp.mpf(0)] * n, [mp.mpf(0)] * n
        dec.ill = False
        carry = mp.mpf(0)   # what the robustness weights hand on: 11 (max|res| / cmad) max unit of the pass before

        def local(i, nleft, nright, robust):
            h = max(xs[i] - xs[nleft], xs[nright] - xs[i])
            w, a, j = {}, mp.mpf(0), nleft
            while j < n:
                r = abs(xs[j] - xs[i])
                if dec.take("r <= h9", r, h * 999 / 1000, u * xmax, le):
                    wj = mp.mpf(1) if dec.take("r <= h1", r, h / 1000, u * xmax, le) else (1 - (r / h) ** 3) ** 3
                    w[j] = wj * rw[j] if robust else wj
                    a += w[j]
                elif xs[j] > xs[i]:
                    break
                j += 1
            base = u * (1 + (xmax / h if h > 0 else 0)) * ymax
            if a <= 0:
                return None, base
            w = {j: v / a for j, v in w.items()}
            if h > 0:
                a = mp.fsum(v * xs[j] for j, v in w.items())
                b = xs[i] - a
                c = mp.fsum(v * (xs[j] - a) ** 2 for j, v in w.items())
                if dec.take("sqrt(c) > .001 range", mp.sqrt(c), rng / 1000, u * xmax, gt):
                    b /= c
                    w = {j: v * (b * (xs[j] - a) + 1) for j, v in w.items()}
            return mp.fsum(v * ys[j] for j, v in w.items()), base

        for it in range(iters + 1):
            dec.passes = it + 1
            nleft, nright, last, i = 0, ns - 1, -1, 0
            while True:
                if nright < n - 1:
                    d1, d2 = xs[i] - xs[nleft], xs[nright + 1] - xs[i]
                    if d1 > d2:   # equal spacing makes this a tie in exact arithmetic; either window holds the same points within h9
                        nleft += 1; nright += 1
                        continue
                v, base = local(i, nleft, nright, it > 0)
                fit[i], unit[i] = (ys[i] if v is None else v), base + carry
                if last < i - 1:
                    den = xs[i] - xs[last]
                    for j in range(last + 1, i):
                        al = (xs[j] - xs[last]) / den
                        fit[j], unit[j] = al * fit[i] + (1 - al) * fit[last], max(unit[i], unit[last])
                last = i
                cut = xs[last] + delta
                i = last + 1
                while i < n:
                    if dec.take("x > last + delta", xs[i], cut, u * xmax, gt):
                        break
                    if xs[i] == xs[last]:
                        fit[i], unit[i] = fit[last], unit[last]
                        last = i
                    i += 1
                i = max(last + 1, i - 1)
                if last >= n - 1:
                    break
            if it == iters:
                break
            res = [abs(a - b) for a, b in zip(ys, fit)]
            sc = mp.fsum(res) / n
            srt = sorted(res)
            cmad = 3 * (srt[n // 2] + srt[n - n // 2 - 1])
            umax = max(unit)
            stop = dec.take("cmad < 1e-7 sc", cmad, sc / 10 ** 7, 6 * umax, lt)
            if cmad <= 6 * NOISE * umax and ymax > 0 and (not stop or dec[-1][1] <= NOISE):
                dec.ill = True   # weights from noise: taken, or stopped only by a comparison that is noise itself
            if stop:
                break
            carry = 11 * (max(res) / cmad if cmad > 0 else 1) * umax
            rw = []
            for r in res:
                if dec.take("r <= c1", r, cmad / 1000, umax, le):
                    rw.append(mp.mpf(1))
                elif dec.take("r <= c9", r, cmad * 999 / 1000, umax, le):
                    rw.append((1 - (r / cmad) ** 2) ** 2)
                else:
                    rw.append(mp.mpf(0))
        return fit, unit, dec


def choose(theta, numRej, readings=None):
    """DESeq2's rule on a numRej profile (ints): returns dict(index (1-based), fit, fit_unit, thresh, thresh_unit, decisions).
    max(numRej) <= 10: index 1.  Otherwise the residuals over numRej > 0 (0 when all are 0), thresh = max(fit) - RMS, the first k
    with numRej[k] > thresh, 1 when there is none."""
    dec = Decisions()
    nr = [int(v) for v in numRej]
    fit, unit, _ = lowess(theta, nr, decisions=dec)
    with mp.workdps(DPS):
        out = dict(fit=fit, fit_unit=unit, decisions=dec, thresh=None, thresh_unit=None, ill=dec.ill, passes=dec.passes)
        dec.append(("max(numRej) <= 10", math.inf))   # integers
        if max(nr) <= 10:
            out["index"] = 1
            return out
        pos = [k for k in range(len(nr)) if nr[k] > 0]
        rms = mp.sqrt(mp.fsum((nr[k] - fit[k]) ** 2 for k in pos) / len(pos))
        thresh, tu = max(fit) - rms, 2 * max(unit)
        above = [k for k in range(len(nr)) if dec.take("numRej > thresh", mp.mpf(nr[k]), thresh, tu, lambda a, b: a > b)]
        out.update(index=above[0] + 1 if above else 1, thresh=thresh, thresh_unit=tu)
        return out


def final_padj(pvalue, passes):
    """padj over the rows with passes[row] True (the IEEE BH sequence), NA elsewhere"""
    sel = [i for i in range(len(pvalue)) if passes[i]]
    adj = bh_ieee([float(pvalue[i]) for i in sel])
    out = [math.nan] * len(pvalue)
    for i, v in zip(sel, adj):
        out[i] = v
    return out


# ---------------------------------------------------------------------------------------------------------------------------
# IHW application (chicdiff.R:2038-2049)
# ---------------------------------------------------------------------------------------------------------------------------
def ihw_groups(avDist, breaks, left_closed=False):
    """group = as.integer(cut(log|avDist|, breaks)): the k (1-based) with b_k < x <= b_(k+1), NA outside, for NaN and where log gives
    NaN.  Returns (group, dist): dist = distance of x to the nearest finite break in ulps of x.  Where x is exact in IEEE arithmetic
    too (log 1 = 0, log 0 = -Inf, log Inf = Inf) nothing is a rounding matter and dist is inf.  left_closed: [b_k, b_(k+1)), a wrong
    reading, for the tests."""
    b = [float(v) for v in breaks]
    seen = {}
    with mp.workdps(DPS):
        bm = [v if math.isinf(v) else mp.mpf(v) for v in b]
        inside = (lambda lo, x, hi: lo <= x < hi) if left_closed else (lambda lo, x, hi: lo < x <= hi)
        for d in set(abs(float(v)) for v in avDist):
            if math.isnan(d):
                seen[d] = (NA_INT, math.inf)
                continue
            exact = d in (0.0, 1.0, math.inf)
            x = -math.inf if d == 0 else math.inf if math.isinf(d) else mp.log(mp.mpf(d))
            g = [k for k in range(len(b) - 1) if inside(bm[k], x, bm[k + 1])]
            if exact:
                dist = math.inf
            else:
                dist = min([float(abs(x - v) / ulp(x)) for v in bm if not isinstance(v, float)] or [math.inf])
            seen[d] = (g[0] + 1 if g else NA_INT, dist)
    groups, dists = [], []
    for v in avDist:
        v = abs(float(v))
        g, d = seen[v] if not math.isnan(v) else (NA_INT, math.inf)
        groups.append(g); dists.append(d)
    return groups, dists


def ihw_weights(groups, avWeights, pvalue):
    """weight = avWeights[group] / mean(avWeights[group]) — no na.rm: one NA group makes every weight NA —, weighted_pvalue = p /
    weight.  Returns (weight, unit) as Fractions (None = NA) and the exact mean (None = NA)."""
    w = [None if g == NA_INT else Fraction(float(avWeights[g - 1])) for g in groups]
    n = len(w)
    if any(v is None for v in w) or any(math.isnan(float(v)) for v in avWeights):
        return [None] * n, [None] * n, None
    mean = sum(w) / n
    if mean == 0:
        return [None] * n, [None] * n, mean   # 0 / 0
    return [v / mean for v in w], [U * (v / mean) * (n + 1) for v in w], mean
