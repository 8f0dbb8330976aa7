"""The normalisation stage — Chicago tables and counts -> the factors the fit divides by — in 50-digit arithmetic (mpmath).

Written from chicdiff.R:538-573 (the refitted distance function), :628-703 and :894-896 (Bmean, Tmean, FullMean per fragment pair),
:1540-1547 (sums by region), :1557-1562 (size factors), :1583-1589, :1614-1615, :1635-1638, :1666-1669 (offsets and the theta mix) and
SURVEY.md (Appendix A1, Appendix B, section 8 a5) — not from the CPU oracle and not from the kernels, and it shares no code with
oracle/, chicdiff_amd/ or the other twins, so tests/test_norm_twin.py and tests/test_gpu_norm.py can hold either of them to something
that has none of their readings of the reference and none of their roundings.

Inputs are the doubles and ints the device gets; from there on every value is an mpf of DPS digits (callers need no workdps: every
function sets it).  A value that IEEE arithmetic makes NaN or +-Inf is a Python float (the pattern is then an exact requirement), a
value that is a pure copy of an input double is that float too (bits are an exact requirement), everything else is an mpf.

UNITS.  u = 2^-53, the relative error of one rounding to nearest.  A quantity's unit is u times its condition with respect to the
roundings a double-precision evaluation MUST make; an evaluation's error is counted in these units and the count of its roundings
(BOUND below) is what it may reach.  A unit of 0 means the value is exact in double arithmetic whichever way it is formed.

  log Bmean   e = e(ld), ld = log|dist| (dist an exact integer).  Rounding ld moves e by |de/dld| |ld| u.  The polynomial (head and
              tail: alpha + beta ld; inside: c0 + c1 ld + c2 ld^2 + c3 ld^3) is a sum whose terms each carry roundings relative to
              themselves: T = sum |terms|.  exp, s_j x, s_i x: one rounding each, relative to Bmean.
                  unit(log Bmean) = u (|de/dld| |ld| + T + 3),     unit(Bmean) = Bmean unit(log Bmean).
              BOUND 8: ld from a 1-ulp log (2 u), each term at most 4 roundings (two products for ld^3, the coefficient, its addition)
              plus the 3 additions' own (7 T u), exp to 1 ulp and the two products (4 u).  The only decisions rounding can flip are ld
              against obs.min / obs.max; the lines continue the cubic with its value and slope (:565-566), so there the two branches
              differ by O((ld - edge)^2) = O(u^2) and the count stands.
  FullMean    Bmean + Tmean, Tmean an exact lookup:  unit = unit(Bmean) + u |FullMean|.  BOUND 8.
  region sum  of F finite doubles: any order of F - 1 additions errs by at most ((1 + u)^(F-1) - 1) sum|x| (= (F-1) u sum|x| to first
              order; relative to the sum that is (F-1) u sum|x| / |sum x|).  That is the unit; BOUND 1.  F = 0 and F = 1: unit 0.
  size factor exp(median_i(log k_ij - mean_j log k_ij)).  With L the largest |log k| over the used rows every key is known to
              about u 2 L whatever row it belongs to, and an order statistic of perturbed keys is within the largest perturbation of the
              same order statistic of the exact keys — so the unit holds whichever row the double-precision select lands on:
                  unit(sf) = sf u (1 + 2 L).
              BOUND (S + 6) / 2 + 3: per key, log k to 1 ulp (2 L u), the S logs of the mean to 1 ulp (2 L u), their S - 1 additions
              ((S-1) L u), the division (L u), the subtraction (2 L u) = (S + 6) L u = (S + 6)/2 units; the mean of two middles 1,
              exp to 1 ulp 2.
  offsets     M3 = x_j / exp(mean_j log x_j).  With Lbar = mean_j |log x_j|:  unit(M3) = M3 u (1 + Lbar).  BOUND S + 2: S logs to 1 ulp
              (2 Lbar u), S - 1 additions ((S-1) Lbar u), / S (Lbar u), exp to 1 ulp (2 u), the quotient (u).
              Mixed: sc = M3 (1 - theta) + sf theta carries M3's error and 4 roundings of its own (no cancellation: all terms are
              positive); sc_j / gm(sc) carries at most twice the row's worst error of sc and the renormalisation's own:
                  unit(mixed) = out u (2 (1 + Lbar(x)) + (1 + Lbar(sc))),   BOUND S + 5
              (Lbar(x) := 0 for a row that took the size factors: they are exact).  Unmixed rows that take the size factors are copies:
              bits.

A row of FullMean is NA for :1588 when M3 has a NaN: an element NaN; negative (log gives NaN, the mean spreads it); 0 (log -Inf, the mean
-Inf, exp 0, 0 / 0); +Inf (Inf / Inf); -Inf (log NaN).  Finite positive rows are never NA as long as exp(mean log) neither overflows nor
underflows — `far_from_overflow` states that about an input, and the inputs modules assert it.
"""
import math

import mpmath as mp

DPS = 50
U = mp.ldexp(mp.mpf(1), -53)

BOUND_LOGB = 8.0
BOUND_FULLMEAN = 8.0
BOUND_SUM = 1.0


def bound_sf(S):
    return (S + 6) / 2.0 + 3.0


def bound_offsets(S, mixed):
    return float(S + 5 if mixed else S + 2)


def special(x):
    """a value held as a Python float: NaN, +-Inf, or an exact copy of an input"""
    return isinstance(x, float)


def round_half_even_half(d2):
    """round(d2 / 2) as R rounds (IEC 60559: halves to even) for an integer d2"""
    q, rem = divmod(int(d2), 2)
    if rem == 0:
        return q
    return q if q % 2 == 0 else q + 1   # d2 / 2 = q + 0.5 lies between q and q + 1


# ---------------------------------------------------------------------------------------------------------------------------
# a3: Bmean, Tmean, FullMean per fragment pair and sample
# ---------------------------------------------------------------------------------------------------------------------------
def _ieee_line(a, b, ld):
    """a + b * ld with ld = -Inf, as IEEE arithmetic (R) gives it"""
    return float(a) + float(b) * ld


def fragment_background(bait, oe, id_min, midsum, sj, si, tblb, tlb, T, distfun):
    """sj, si, tblb, tlb: (S, nid); T: (S, ntblb, ntlb), NaN = a (tblb, tlb) pair never observed; distfun: (S, 10) = cubic c0..c3,
    head alpha, beta, tail alpha, beta, obs.min, obs.max.  Returns a dict of (S, nru) nested lists:
      B, F        mpf, or a float where the value is NaN / Inf / an exact 0;   uB, uF   their units (mpf; 0 where exact)
      T           floats (a lookup: bits)
      dist        per row: the rounded distance, None off the map;   cls   per row and sample: "off map", "dist 0", "head", "cubic", "tail"
    """
    S, nid = len(sj), len(midsum)
    nru = len(bait)
    nan = float("nan")
    out = dict(B=[[nan] * nru for _ in range(S)], uB=[[mp.mpf(0)] * nru for _ in range(S)], T=[[nan] * nru for _ in range(S)],
               F=[[nan] * nru for _ in range(S)], uF=[[mp.mpf(0)] * nru for _ in range(S)], dist=[None] * nru,
               cls=[["off map"] * nru for _ in range(S)])
    with mp.workdps(DPS):
        par = [[mp.mpf(float(v)) for v in distfun[s]] for s in range(S)]
        lowest = []   # :689-692: the lowest observed Tmean of every tblb
        for s in range(S):
            row = []
            for tb in range(len(T[s])):
                seen = [float(v) for v in T[s][tb] if not math.isnan(float(v))]
                row.append(min(seen) if seen else nan)
            lowest.append(row)
        for r in range(nru):
            b, o = int(bait[r]) - int(id_min), int(oe[r]) - int(id_min)
            if not (0 <= b < nid and 0 <= o < nid):
                continue
            dist = round_half_even_half(int(midsum[o]) - int(midsum[b]))   # :648
            out["dist"][r] = dist
            ld = mp.log(abs(dist)) if dist != 0 else None
            for s in range(S):
                c0, c1, c2, c3, ha, hb, ta, tb_, omin, omax = par[s]
                if ld is None:
                    cls = "dist 0"   # log(0) = -Inf < obs.min: the head line
                    e = _ieee_line(distfun[s][4], distfun[s][5], -math.inf)
                    f = nan if math.isnan(e) else math.inf if e > 0 else 0.0   # exp(+-Inf)
                    ulog = mp.mpf(0)
                else:
                    if ld > omax:
                        cls, e, slope, terms = "tail", ta + tb_ * ld, tb_, abs(ta) + abs(tb_ * ld)
                    elif ld < omin:
                        cls, e, slope, terms = "head", ha + hb * ld, hb, abs(ha) + abs(hb * ld)
                    else:
                        l2 = ld * ld
                        cls, e, slope = "cubic", c0 + c1 * ld + c2 * l2 + c3 * l2 * ld, c1 + 2 * c2 * ld + 3 * c3 * l2
                        terms = abs(c0) + abs(c1 * ld) + abs(c2 * l2) + abs(c3 * l2 * ld)
                    f = mp.exp(e)
                    ulog = U * (abs(slope) * abs(ld) + terms + 3)
                out["cls"][s][r] = cls
                a_j, a_i = float(sj[s][b]), float(si[s][o])
                if math.isnan(a_i):
                    a_i = 1.0                                             # :672
                assert math.isfinite(a_i) and (math.isnan(a_j) or math.isfinite(a_j)), "s_j, s_i: finite or NA"
                if math.isnan(a_j):
                    B, uB = nan, mp.mpf(0)                                # :702
                elif special(f):
                    B, uB = a_j * a_i * f, mp.mpf(0)                      # Inf * x, 0 * x as IEEE has them
                else:
                    B = mp.mpf(a_j) * mp.mpf(a_i) * f
                    uB = abs(B) * ulog
                kb, kl = int(tblb[s][b]), int(tlb[s][o])
                if kb < 0:
                    Tm = nan
                elif kl >= 0:
                    Tm = float(T[s][kb][kl])
                else:
                    Tm = lowest[s][kb]
                if special(B) or math.isnan(Tm):
                    F, uF = (B if special(B) else 0.0) + Tm, mp.mpf(0)
                else:
                    F = B + mp.mpf(Tm)
                    uF = uB + U * abs(F)
                out["B"][s][r], out["uB"][s][r], out["T"][s][r], out["F"][s][r], out["uF"][s][r] = B, uB, Tm, F, uF
    return out


# ---------------------------------------------------------------------------------------------------------------------------
# a2: sums by region
# ---------------------------------------------------------------------------------------------------------------------------
def window_sums(fragN, fragFM, region_ptr):
    """fragN (nfrag, S) ints or None, fragFM (nfrag, S) doubles or None, region_ptr (n + 1).  Returns (N, FM, uFM): (n, S) nested lists;
    N Python ints; FM mpf or a float (NaN if any term is NaN — there is no na.rm —, +-Inf as IEEE adds, 0.0 for an empty region), uFM
    the unit."""
    n = len(region_ptr) - 1
    N = FM = uFM = None
    with mp.workdps(DPS):
        if fragN is not None:
            S = len(fragN[0]) if len(fragN) else 0
            N = [[sum(int(fragN[f][j]) for f in range(int(region_ptr[i]), int(region_ptr[i + 1]))) for j in range(S)] for i in range(n)]
        if fragFM is not None:
            S = len(fragFM[0]) if len(fragFM) else 0
            FM, uFM = [[0.0] * S for _ in range(n)], [[mp.mpf(0)] * S for _ in range(n)]
            for i in range(n):
                lo, hi = int(region_ptr[i]), int(region_ptr[i + 1])
                if hi == lo:
                    continue
                grow = (1 + U) ** (hi - lo - 1) - 1
                for j in range(S):
                    x = [float(fragFM[f][j]) for f in range(lo, hi)]
                    if any(math.isnan(v) for v in x):
                        FM[i][j] = float("nan")
                    elif any(math.isinf(v) for v in x):
                        FM[i][j] = sum(v for v in x if math.isinf(v))   # Inf + finite = Inf; Inf - Inf = NaN
                    else:
                        FM[i][j] = mp.fsum(mp.mpf(v) for v in x)
                        uFM[i][j] = grow * mp.fsum(abs(mp.mpf(v)) for v in x)
    return N, FM, uFM


# ---------------------------------------------------------------------------------------------------------------------------
# a5: size factors
# ---------------------------------------------------------------------------------------------------------------------------
def size_factors(counts):
    """counts (n, S) ints (NA_integer_ = INT_MIN).  A row is used when every count is > 0.  Returns (sf, unit, used): S mpf each, and
    the number of used rows; sf is None when there is none."""
    with mp.workdps(DPS):
        S = len(counts[0])
        logs = {}
        keys = [[] for _ in range(S)]
        L = mp.mpf(0)
        for row in counts:
            k = [int(v) for v in row]
            if min(k) <= 0:
                continue
            l = []
            for v in k:
                if v not in logs:
                    logs[v] = mp.log(v)
                l.append(logs[v])
            lg = mp.fsum(l) / S
            L = max([L] + [abs(v) for v in l])
            for j in range(S):
                keys[j].append(l[j] - lg)
        m = len(keys[0])
        if m == 0:
            return None, None, 0
        sf = []
        for j in range(S):
            ks = sorted(keys[j])
            med = ks[m // 2] if m % 2 else (ks[m // 2 - 1] + ks[m // 2]) / 2
            sf.append(mp.exp(med))
        return sf, [v * U * (1 + 2 * L) for v in sf], m


# ---------------------------------------------------------------------------------------------------------------------------
# a4: offsets
# ---------------------------------------------------------------------------------------------------------------------------
def row_is_na(row):
    """:1586-1588 on one row of FullMean (see the module's docstring)"""
    return any(math.isnan(v) or math.isinf(v) or v <= 0 for v in (float(x) for x in row))


def far_from_overflow(FM, lo=1e-250, hi=1e250):
    """True when every finite positive element lies in [lo, hi]: then exp(mean log) and every quotient stay normal, and "is this row
    NA" is no rounding decision."""
    return all(lo <= float(v) <= hi for row in FM for v in row if math.isfinite(float(v)) and float(v) > 0)


def _geo(vals):
    l = [mp.log(v) for v in vals]
    return mp.exp(mp.fsum(l) / len(l)), mp.fsum(abs(v) for v in l) / len(l)


def offsets(FM, sf, theta=None, norm="combined"):
    """FM (n, S) doubles, sf S doubles, theta None or a double.  Returns (out, unit, na): (n, S) nested lists and the rows that took
    the size factors.  norm = "standard": the size factors in every row; theta None: normFactorsM3 (norm = "fullmean")."""
    S = len(sf)
    fs = [float(v) for v in sf]
    zero = mp.mpf(0)
    out, unit, na = [], [], []
    with mp.workdps(DPS):
        ms = [mp.mpf(v) for v in fs]
        th = None if theta is None else mp.mpf(float(theta))
        for row in FM:
            if norm == "standard":
                out.append(list(fs)); unit.append([zero] * S); na.append(False)
                continue
            isna = row_is_na(row)
            na.append(isna)
            if isna:
                m3, lbar1 = ms, zero
            else:
                x = [mp.mpf(float(v)) for v in row]
                g, lbar1 = _geo(x)
                m3 = [v / g for v in x]
            if th is None:
                out.append(list(fs) if isna else m3)
                unit.append([zero] * S if isna else [v * U * (1 + lbar1) for v in m3])
                continue
            sc = [a * (1 - th) + b * th for a, b in zip(m3, ms)]     # :1635 / :1666
            g, lbar2 = _geo(sc)
            res = [v / g for v in sc]                                # :1638 / :1669
            out.append(res)
            unit.append([v * U * (2 * (1 + lbar1) + (1 + lbar2)) for v in res])
    return out, unit, na


# ---------------------------------------------------------------------------------------------------------------------------
# .chicEstimateDistFun, second half (:548-569)
# ---------------------------------------------------------------------------------------------------------------------------
def distfun_fit(values, binsize=20000):
    """The exact least-squares cubic of log(values) on log(midpoint) and the two lines that continue it.  Returns a dict: params (ten
    mpf, the layout of `distfun` above), x (the log midpoints), curve(ld) -> (value, condition): the fitted function at ld and the
    condition of that value — by how much it can move per unit of relative perturbation of size 1 of each column of the design matrix
    (in its 2-norm), of the data (2-norm) and of the terms of its own evaluation:
        ||h|| (sum_k |c_k| ||a_k|| + ||y||) + ||r|| sum_k |g_k| ||a_k|| + sum |terms|,
    h = A (A'A)^-1 a(ld) the weights of the data in the value, g = (A'A)^-1 a(ld), r the residuals (first-order perturbation of a
    least-squares solution, Higham, Accuracy and Stability of Numerical Algorithms, section 20.1)."""
    with mp.workdps(2 * DPS):   # the normal equations of a cubic in log d lose ~ 15 digits
        n = len(values)
        half = round_half_even_half(int(binsize))
        x = [mp.log(half + int(binsize) * i) for i in range(n)]
        y = [mp.log(mp.mpf(float(v))) for v in values]
        A = mp.matrix([[1, t, t * t, t * t * t] for t in x])
        AtA = A.T * A
        inv = mp.inverse(AtA)
        c = inv * (A.T * mp.matrix(y))
        r = mp.matrix(y) - A * c
        cn = [mp.norm(A[:, k]) for k in range(4)]
        yn, rn = mp.norm(mp.matrix(y)), mp.norm(r)
        c = [c[k] for k in range(4)]
        ends = [min(x), max(x)]
        beta = [c[1] + 2 * c[2] * t + 3 * c[3] * t * t for t in ends]                        # :565
        alpha = [c[0] + (c[1] - b) * t + c[2] * t * t + c[3] * t ** 3 for b, t in zip(beta, ends)]  # :566

        def curve(ld):
            with mp.workdps(2 * DPS):
                ld = mp.mpf(ld)
                a0 = mp.matrix([1, ld, ld * ld, ld ** 3])
                if ld < ends[0] or ld > ends[1]:
                    t = ends[0] if ld < ends[0] else ends[1]
                    a0 = mp.matrix([1, t, t * t, t ** 3]) + (ld - t) * mp.matrix([0, 1, 2 * t, 3 * t * t])   # value + slope (ld - t): linear in c
                g = inv * a0
                h = A * g
                val = mp.fsum(a0[k] * c[k] for k in range(4))
                cond = (mp.norm(h) * (mp.fsum(abs(c[k]) * cn[k] for k in range(4)) + yn)
                        + rn * mp.fsum(abs(g[k]) * cn[k] for k in range(4)) + mp.fsum(abs(a0[k] * c[k]) for k in range(4)))
                return val, cond

        return dict(params=[*c, alpha[0], beta[0], alpha[1], beta[1], ends[0], ends[1]], x=x, curve=curve)
