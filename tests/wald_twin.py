"""The Wald stage (nbinomWaldTest for the designs ~condition with two levels and ~1) in 50-digit arithmetic (mpmath).

Written from SURVEY.md Appendix A5 and the column descriptions of include/chicdiff_hip.h — not from the CPU oracle and not from the
kernels — so that tests/test_wald_twin.py and tests/test_gpu_wald.py can hold either of them to something that shares no code and
no rounding with it.  Two functions:

  closed_forms(...)  everything that is a closed form of a row's inputs and the reported (dispersion, intercept, lfc): both standard
                     errors, stat, p, the hat diagonals, the robust dispersion, Cook's distances, their maximum and its position —
                     and the units in which an error of each is counted;
  replay(...)        the ridge IRLS from the least-squares start, step by step, with DESeq2's stopping rule.

Every value returned is an mpf of DPS digits; callers work inside `with mp.workdps(DPS)` (mpmath rounds the RESULT of an operation to
the precision in force where the operation runs, so 50-digit operands combined outside it give 15 digits).  replay() carries its
recursion in 224-bit fixed point (57 digits or more of every quantity that matters, see there) and hands back mpf values.

Constants are the doubles DESeq2 computes with (0.5, 0.04, 0.1, the trim scales 2.04 / 1.86 / 1.51, betaTol); the ridge 1e-6 / ln(2)^2 is
formed exactly (a rounding of it would change a standard error by 1e-23 relative).
"""
import mpmath as mp
import numpy as np
from mpmath import libmp

DPS = 50
U = mp.ldexp(mp.mpf(1), -52)


def _lam():
    return mp.mpf(10) ** -6 / mp.log(2) ** 2  # the ridge: 1e-6 on the log2 scale, on every coefficient


def trim_class(n):
    """(values dropped at each end, scale) of DESeq2's trimmedCellVariance for a cell of n samples: trim ratio 1/3, 1/4, 1/8 and scale
    2.04, 1.86, 1.51 on the bins (0, 3.5], (3.5, 23.5], (23.5, Inf); R's mean(x, trim) drops floor(n trim) values at each end."""
    if n <= 3:
        return n // 3, 2.04
    if n <= 23:
        return n // 4, 1.86
    return n // 8, 1.51


def robust_dispersion(q, g):
    """alpha_rob = max((v - m) / m^2, 0.04) with m the mean of q and v the largest scaled trimmed cell variance over cells of >= 3
    samples.  Returns (alpha_rob, v, m, c_v); c_v = sum_kept 2 |q - c| (|q| + |c|) / sum_kept (q - c)^2 measures the cancellation inside
    the kept squares of the cell that gives v (0 when they are all zero).  None when no cell has 3 samples."""
    m = mp.fsum(q) / len(q)
    best = None
    for c in (0, 1):
        cell = [x for x, gj in zip(q, g) if gj == c]
        n = len(cell)
        if n < 3:
            continue
        lo, scale = trim_class(n)
        s = sorted(cell)
        cbar = mp.fsum(s[lo:n - lo]) / (n - 2 * lo)
        sq = sorted(((x - cbar) ** 2, x) for x in cell)  # equal squares are interchangeable: the kept sum does not depend on the tie-break
        kept = sq[lo:n - lo]
        ssum = mp.fsum(d for d, _ in kept)
        v = mp.mpf(scale) * ssum / (n - 2 * lo)
        cv = mp.fsum(2 * abs(x - cbar) * (abs(x) + abs(cbar)) for _, x in kept) / ssum if ssum != 0 else mp.mpf(0)
        if best is None or v > best[0]:
            best = (v, cv)
    if best is None:
        return None
    v, cv = best
    arob = (v - m) / (m * m)
    floor = mp.mpf(0.04)
    return (arob if arob > floor else floor), v, m, cv


def closed_forms(y, nf, group, alpha, intercept, lfc, optim_path=False):
    """The Wald outputs of one row as functions of its counts y, offsets nf, the design, and the REPORTED dispersion, intercept and
    log2 fold change (doubles, taken as exact).  `optim_path` is accepted for symmetry with the fit (rows that left the IRLS for the
    optimiser): it changes only the mu of the reported deviance, which tests/test_gpu_objective.py covers, so nothing returned here
    depends on it.

    Returns a dict: interceptSE, lfcSE, stat, maxCooks (None = NaN), cooksArgmax, tie (the first maximum has an exact equal), cooks
    (per sample; None when no cell has 3 samples), hat, floored (samples with nf e^eta < 0.5), kappa, se_unit, cooks_unit ({sample: unit} for the
    two samples a caller needs, the counted maximum and the first maximum; None where y == mu_f exactly: no relative error there), beta_unit, betaIter (1 for ~1, else None), intercept (~1 only)."""
    S = len(y)
    g = [int(v != 0) for v in group]
    al = mp.mpf(float(alpha))
    ln2 = mp.log(2)
    log2e = 1 / ln2
    yv = [mp.mpf(int(v)) for v in y]
    fv = [mp.mpf(float(v)) for v in nf]
    qv = [a / b for a, b in zip(yv, fv)]
    if not any(g):  # design ~1: fitNbinomGLMs' shortcut
        b0 = mp.log(mp.fsum(qv) / S) / ln2
        e = mp.power(2, mp.mpf(float(intercept)))
        xtwx = mp.fsum(1 / (1 / (f * e) + al) for f in fv)
        se = log2e / mp.sqrt(xtwx)
        return dict(intercept=b0, interceptSE=se, lfcSE=None, stat=mp.mpf(float(intercept)) / se, maxCooks=None, cooksArgmax=-1, tie=False,
                    cooks=None, hat=None, floored=0, kappa=mp.mpf(1), se_unit=U, cooks_unit=None, betaIter=1,
                    beta_unit=U * max(mp.mpf(1), abs(b0)))
    B0, B1 = mp.mpf(float(intercept)), mp.mpf(float(lfc))
    E = (mp.exp(B0 * ln2), mp.exp((B0 + B1) * ln2))
    half = mp.mpf(0.5)
    muf = [f * E[gj] for f, gj in zip(fv, g)]
    mu = [m if m > half else half for m in muf]
    w = [m / (1 + al * m) for m in mu]
    wA = mp.fsum(x for x, gj in zip(w, g) if not gj)
    wB = mp.fsum(x for x, gj in zip(w, g) if gj)
    lam = _lam()
    m00, m01, m11 = wA + wB + lam, wB, wB + lam
    det = m00 * m11 - m01 * m01
    i00, i01, i11 = m11 / det, -m01 / det, m00 / det
    a00, a01, a11 = wA + wB, wB, wB
    t00, t01 = i00 * a00 + i01 * a01, i00 * a01 + i01 * a11
    t10, t11 = i01 * a00 + i11 * a01, i01 * a01 + i11 * a11
    v0, v1 = t00 * i00 + t01 * i01, t10 * i01 + t11 * i11
    se0, se1 = log2e * mp.sqrt(v0), log2e * mp.sqrt(v1)
    kappa = (m00 * m11 + m01 * m01) / det
    xmx = (i00, i00 + 2 * i01 + i11)
    hat = [x * xmx[gj] for x, gj in zip(w, g)]
    out = dict(interceptSE=se0, lfcSE=se1, stat=B1 / se1, hat=hat, floored=sum(1 for m in muf if m < half), kappa=kappa, se_unit=U * kappa,
               beta_unit=U * max(mp.mpf(1), abs(B0), abs(B1)), betaIter=None, maxCooks=None, cooksArgmax=-1, tie=False, cooks=None,
               cooks_unit=None)
    rob = robust_dispersion(qv, g)
    if rob is None:
        return out
    arob, v, m, cv = rob
    size = [g.count(0), g.count(1)]
    cooks = []
    for yj, mf, h in zip(yv, muf, hat):
        r = yj - mf
        cooks.append(r * r / (mf + arob * mf * mf) / 2 * h / (1 - h) ** 2)

    def unit_of(j):
        yj, mf, h = yv[j], muf[j], hat[j]
        r = yj - mf
        if r == 0:
            return None
        t = 1 + 2 * (yj + mf) / abs(r) + kappa * (1 + 2 * h / (1 - h))
        if arob > mp.mpf(0.04):
            t += (arob * mf * mf / (mf + arob * mf * mf)) * ((v * (1 + cv) + m) / abs(v - m) + 2)
        return U * t

    top = max(cooks)
    first = cooks.index(top)
    counted = [j for j in range(S) if size[g[j]] >= 3]
    jmax = max(counted, key=lambda j: (cooks[j], -j))
    out.update(cooks=cooks, cooks_unit={j: unit_of(j) for j in {jmax, first}}, maxCooks=cooks[jmax], maxCooksAt=jmax, cooksArgmax=first, tie=cooks.count(top) > 1,
               alpha_rob=arob)
    return out


def p_two_sided(stat):
    """2 Phi(-|stat|) at the reported stat."""
    return mp.erfc(abs(mp.mpf(float(stat))) / mp.sqrt(2))


_LGAMMA1 = {}


def _lfact(y):
    v = _LGAMMA1.get(y)
    if v is None:
        v = _LGAMMA1[y] = mp.loggamma(mp.mpf(y) + 1)
    return v


P = 224            # fractional bits of replay()'s fixed-point numbers: 2^-224 = 3.7e-68 absolute
_ONE = 1 << P


def _fx(x):
    """mpf -> fixed point (an int, in units of 2^-P)."""
    return int(mp.floor(mp.ldexp(x, P)))


def _mp(v):
    """fixed point -> mpf (rounded to the precision in force)."""
    return mp.ldexp(mp.mpf(v), -P)


def _log_fx(t):
    """log of a positive fixed-point number, fixed point (mpmath's logarithm at P + 8 bits, without the detour over mpf objects)."""
    return libmp.to_fixed(libmp.mpf_log(libmp.from_man_exp(t, -P), P + 8, "n"), P)


_ROWS = {}


def _row_logs(y, nf):
    """(offsets, log offsets, log(q + 0.1)) of a row in fixed point; kept, since a row is replayed for more than one dispersion."""
    key = (bytes(memoryview(y)), bytes(memoryview(nf)))
    if key not in _ROWS:
        fv = [mp.mpf(float(v)) for v in nf]
        _ROWS[key] = ([_fx(f) for f in fv], [_fx(mp.log(f)) for f in fv], [_fx(mp.log(int(a) / f + mp.mpf(0.1))) for a, f in zip(y, fv)])
    return _ROWS[key]


def replay(y, nf, group, alpha, maxit=100, tol=1e-8, extra=0):
    """The ridge IRLS of one ~condition row from the least-squares start beta_0 = (mean_A log(q + 0.1), mean_B - mean_A).  Tick k takes
    the ridge-WLS step from beta_k with mu = max(nf e^eta, 0.5), w = mu / (1 + alpha mu), z = log(mu / nf) + (y - mu) / mu; from k >= 1 it
    first forms the deviance at beta_k (floored mu) and conv_test = |dev - dev_old| / (|dev| + 0.1).  It stops at the first k >= 2 with
    conv_test < tol, at k = maxit, or when a |beta| exceeds 30: the row then counts as maxit (DESeq2 hands it to optim).
    Returns dict(stop, optim, betas = [(b0, b1)] natural scale, beta_0 .. at least beta_stop, conv = [None, conv_test(1), ...]); after a
    stop by convergence the trace goes on for `extra` ticks, so that a fit that stopped one step later can be compared with it.

    The recursion itself runs on Python integers in units of 2^-P (a sum is exact, a product or quotient is off by less than one unit,
    3.7e-68: every quantity of the recursion that matters is above 1e-10 in magnitude, so this is 57 digits or more; mpmath's own
    numbers cost ten times as much per operation, and this loop is S x steps x rows long).  exp and log are mpmath's, at 68 digits.
    Written as w z = w (eta - 1) + y / (1 + alpha mu), which is the same number."""
    g = [int(v != 0) for v in group]
    nA, nB = g.count(0), g.count(1)
    with mp.workdps(68):
        al_m = mp.mpf(float(alpha))
        r_m = 1 / al_m
        ys = [int(v) for v in y]
        f_x, lf, l = _row_logs(np.ascontiguousarray(y, dtype=np.int64), np.ascontiguousarray(nf, dtype=np.float64))
        al, r = _fx(al_m), _fx(r_m)
        tenth, half, lhalf, lam = _fx(mp.mpf(0.1)), _ONE >> 1, _fx(mp.log(mp.mpf(0.5))), _fx(_lam())
        tol_x, thirty = _fx(mp.mpf(float(tol))), 30 * _ONE
        # the part of sum_j log dnbinom(y_j; size r, mu_j) that does not depend on beta: lgamma(y + r) - lgamma(r) - lgamma(y + 1) + y log alpha
        # (30 digits: a constant of the row, which cancels in dev - dev_old and is left only in the |dev| + 0.1 that scales conv_test)
        with mp.workdps(30):
            lgr, la = mp.loggamma(r_m), mp.log(al_m)
            const = _fx(mp.fsum(mp.loggamma(a + r_m) - lgr - _lfact(a) + a * la for a in ys if a != 0))
        b0 = sum(x for x, gj in zip(l, g) if not gj) // nA
        b1 = sum(x for x, gj in zip(l, g) if gj) // nB - b0
        ra = [r + a * _ONE for a in ys]
        ylf = sum(a * x for a, x in zip(ys, lf))  # sum_j y_j log nf_j
        betas, conv = [(b0, b1)], [None]
        dev_old = 0
        stop, optim, k, left = None, False, 0, extra
        while True:
            eta = (b0, b0 + b1)
            E = (_fx(mp.exp(_mp(eta[0]))), _fx(mp.exp(_mp(eta[1]))))
            wA = wB = zA = zB = ll = 0
            for a, f, lfj, raj, gj in zip(ys, f_x, lf, ra, g):
                m = (f * E[gj]) >> P
                if m < half:
                    m, ej = half, lhalf - lfj  # eta of the floored mu: log(mu / nf)
                else:
                    ej = eta[gj]
                t = _ONE + ((al * m) >> P)
                w = (m << P) // t
                wz = ((w * (ej - _ONE)) >> P) + ((a << (2 * P)) // t if a else 0)
                if gj:
                    wB += w
                    zB += wz
                else:
                    wA += w
                    zA += wz
                if k >= 1:
                    ll += a * ej - ((raj * _log_fx(t)) >> P)
            if k >= 1:
                dev = -2 * (const + ylf + ll)
                c = (abs(dev - dev_old) << P) // (abs(dev) + tenth)
                conv.append(c)
                dev_old = dev
                if stop is None:
                    if k >= 2 and c < tol_x:
                        stop, optim = k, k >= maxit
                    elif k >= maxit:
                        stop, optim = maxit, True
                if stop is not None:
                    if optim or left == 0:
                        break
                    left -= 1
            m00, m01, m11 = wA + wB + lam, wB, wB + lam
            r0, r1 = zA + zB, zB
            det = m00 * m11 - m01 * m01
            b0, b1 = ((m11 * r0 - m01 * r1) << P) // det, ((m00 * r1 - m01 * r0) << P) // det
            k += 1
            betas.append((b0, b1))
            if stop is None and (abs(b0) > thirty or abs(b1) > thirty):
                stop, optim = maxit, True
                break
    return dict(stop=stop, optim=optim, betas=[(_mp(u), _mp(v)) for u, v in betas], conv=[None if c is None else _mp(c) for c in conv])
