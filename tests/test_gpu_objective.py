"""The functions the fits are built from, each against 50-digit arithmetic (mpmath).

tests/test_gpu_parity.py compares finished fits with the CPU oracle to 1e-6 and sends the rows outside to a referee; an objective
wrong at 1e-10 would only lengthen the referee's list.  Here the pieces are measured on their own:

  1. the dispersion objective (eval_point / eval_point_spread behind chicdiff_hip_selftest_objective_dev): log posterior of
     log(alpha) and its derivative at designed points, in units of u T (u = 2^-52, T = the sum of the absolute values of the
     objective's terms BEFORE they cancel), stratified by decade of alpha and S; the GPU's worst error in a stratum must stay within
     4 x the worst error the oracle's own objective makes on the same points in the same run.  (4: the kernel's log, exp and
     reciprocal are 1-ulp functions where libm's are ~1/2 ulp, it splits log(mu + r) = L - a, and it folds the samples in another
     order.)  Every evaluation layout must return the same bits.
  2. the building blocks (chicdiff_hip_selftest_math_dev / _math3_dev): lgamma differences, log1p forms, reciprocals, Stirling
     series, the table-driven log and exp at their table-cell edges, pnorm over its whole domain.
  3. the reported deviance, rebuilt from the fit's own dispersion and coefficients.

Every comparison goes to test_gpu_parity.PARITY_LOG, which tests/conftest.py writes out when the pytest run ends
(profiles/r13_objective_accuracy.json holds the records of one run).
"""
import math

import mpmath as mp
import numpy as np
import pytest

import test_gpu_parity as tgp
from chicdiff_amd import synth

pytestmark = pytest.mark.gpu

U = 2.0 ** -52


@pytest.fixture(scope="module")
def ctx():
    import __graft_entry__ as g
    g.build()  # no-op when the in-tree library and the oracle are up to date
    from chicdiff_amd import hip
    c = hip.HipContext(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def oracle():
    from oracle import oracle as o
    return o


@pytest.fixture(autouse=True)
def _digits():
    with mp.workdps(60):
        yield


def log_record(test, quantity, stratum, points, gpu_worst, yardstick, allowance):
    """One comparison: the GPU's worst error, what it is measured against, and the bound that follows."""
    tgp.PARITY_LOG.append(dict(test=test, quantity=quantity, stratum=stratum, points=int(points), gpu_worst=float(gpu_worst),
                               yardstick=None if yardstick is None else float(yardstick), allowance=float(allowance)))
    print(f"{test} | {quantity} | {stratum}: n={points} GPU worst {gpu_worst:.4g}, yardstick {yardstick}, allowed {allowance:.4g}")


def ulp_of(t):
    """ulp of the double nearest below |t| in magnitude class: 2^(floor(log2 |t|) - 52), 2^-1074 in the subnormal range."""
    e = mp.frexp(t)[1] - 1
    return mp.ldexp(mp.mpf(1), max(int(e), -1022) - 52)


def ulp_errors(got, ref):
    """|got - ref| in ulps of the true value ref (mpf), element by element; both must be finite."""
    out = np.empty(len(ref))
    for i, (g, t) in enumerate(zip(got, ref)):
        assert math.isfinite(g), (i, g, t)
        out[i] = 0.0 if (t == 0 and g == 0) else float(abs(mp.mpf(float(g)) - t) / ulp_of(t if t != 0 else mp.mpf(float(g))))
    return out


def dev(ctx, a):
    import torch
    return torch.as_tensor(np.ascontiguousarray(a, dtype=np.float64)).to(ctx.device)


def bits(x):
    return np.ascontiguousarray(x, dtype=np.float64).view(np.uint64)


# ---------------------------------------------------------------------------------------------------------------------------
# 1. the objective
# ---------------------------------------------------------------------------------------------------------------------------
def eval_points(S):
    """log(alpha) of the designed points: decades down to the grid's floor, both sides of every r = 1/alpha = 10 - k (where the
    number nr of unit steps that lift r to >= 10 changes, and with it `yi > nr`, the profile masks and the prefix table's length),
    0.5, 1, the largest dispersion of a fit (max(10, S)), and the widest the searches evaluate: both line searches clamp a step to
    [-30, 10]; the grid fallback stays inside (log(1e-8) - step .. log(maxDisp) + step, step = (log(maxDisp) - log(1e-8)) / 19)."""
    a = [math.log(v) for v in (1e-8, 1e-6, 1e-4, 1e-2, 0.5, 1.0, float(max(10, S)))]
    for k in range(10):
        c = math.log(1.0 / (10 - k))
        a += [np.nextafter(c, -np.inf), c, np.nextafter(c, np.inf)]
    a += [-30.0, 10.0]
    return np.array(a, dtype=np.float64)


def design_rows(S, two_groups, rng):
    """Base rows (counts, nf): count ramps that put 0 .. 12 next to every nr, the sizes at which the kernels switch method (255 / 256,
    1023 / 1024, 1e6, 2^31 - 1), single nonzeros, one group entirely zero (mu = minmu there), Poisson bulk."""
    small = S < 12
    rows = []
    for off in ((0, 3, 6, 9) if small else (0, 6)):
        rows.append([(off + j) % 13 for j in range(S)])
    big = [255, 256, 10 ** 6, 2 ** 31 - 1, 1023, 1024, 0, 1]
    for off in ((0, 3, 6) if S < 8 else (0,)):
        rows.append([big[(off + j) % 8] for j in range(S)])
    one = [0] * S
    one[0] = 1
    rows.append(one)
    huge = [0] * S
    huge[S - 1] = 2 ** 31 - 1
    rows.append(huge)
    gz = [int(v) for v in rng.poisson(40.0, S)]
    if two_groups:
        for j in range(S // 2, S):
            gz[j] = 0  # group B entirely zero
    gz[0] = max(gz[0], 1)
    rows.append(gz)
    for m in ((5.0, 300.0) if small else (30.0,)):
        r = [int(v) for v in rng.poisson(m, S)]
        r[0] = max(r[0], 1)
        rows.append(r)
    counts = np.array(rows, dtype=np.int64)
    assert counts.max() <= 2 ** 31 - 1 and (counts.sum(axis=1) > 0).all()
    nf = np.exp(rng.uniform(math.log(0.5), math.log(2.0), counts.shape))
    return counts.astype(np.int32), nf


def mp_objective(a, y, mu, g, p2):
    """(lp, T_lp, dlp, T_dlp) without prior, in mpmath.  T: sum of the absolute values of the terms before cancellation — lgamma(y + r)
    and lgamma(r) separately; for the derivative r psi(r) and r psi(y + r) separately."""
    a = mp.mpf(float(a))
    al = mp.exp(a)
    r = 1 / al
    lg_r, dg_r = mp.loggamma(r), mp.digamma(r)
    w = [mp.mpf(0), mp.mpf(0)]
    dw = [mp.mpf(0), mp.mpf(0)]
    ll = T = s = Ts = mp.mpf(0)
    for yj, mj, gj in zip(y, mu, g):
        yj, mj = mp.mpf(int(yj)), mp.mpf(float(mj))
        t = 1 / mj + al
        k = 1 if (p2 and gj) else 0
        w[k] += 1 / t
        dw[k] += -1 / (t * t)
        ma = mj * al
        L = mp.log1p(ma)
        lgy = mp.loggamma(yj + r) if yj else lg_r
        dgy = mp.digamma(yj + r) if yj else dg_r
        t2, t3 = yj * mp.log(mj + r), r * L
        ll += lgy - lg_r - t2 - t3
        T += abs(lgy) + abs(lg_r) + abs(t2) + abs(t3)
        q1, q2 = ma / (1 + ma), yj / (mj + r)
        s += dg_r + L - q1 - dgy + q2
        Ts += abs(dg_r) + abs(L) + abs(q1) + abs(dgy) + abs(q2)
    if p2:
        cr = -mp.mpf(0.5) * mp.log(w[0] * w[1])
        dcr = -mp.mpf(0.5) * (dw[0] / w[0] + dw[1] / w[1])
        Tdcr = mp.mpf(0.5) * (abs(dw[0] / w[0]) + abs(dw[1] / w[1]))
    else:
        cr = -mp.mpf(0.5) * mp.log(w[0])
        dcr = -mp.mpf(0.5) * (dw[0] / w[0])
        Tdcr = abs(dcr)
    return ll + cr, T + abs(cr), r * s + dcr * al, r * Ts + Tdcr * al


# lanes per row the line search gives a row when `live` rows are left in a wave (disp_fit_kernel: the first power of two >= S, two
# at least, halved at most twice and never below two lanes — the most that still holds every live row), written out by hand
LAYOUTS = {3: {16: 4, 32: 2}, 4: {16: 4, 32: 2}, 5: {8: 8, 16: 4, 32: 2}, 8: {8: 8, 5: 8, 16: 4, 11: 4, 32: 2},
           12: {4: 16, 8: 8, 16: 4}, 16: {4: 16, 8: 8, 16: 4}, 33: {1: 64, 2: 32, 4: 16}, 64: {1: 64, 2: 32, 4: 16}}
TOO_MANY = {3: 33, 4: 33, 5: 33, 8: 33, 12: 17, 16: 17, 33: 5, 64: 5}  # one live row more than any layout holds


@pytest.mark.parametrize("S", [3, 4, 5, 8, 12, 16, 33, 64])
def test_objective_against_50_digits(ctx, oracle, S):
    """lp, dlp, alpha and mu of the device objective at the designed points: all four fixed row loaders (S = 4, 8, 12, 16) and the
    generic one, one and two exchange rounds of the samples-across-lanes layout (S R <= 128 and > 128), designs ~condition and ~1,
    with and without prior.  Bound: see the module docstring; nothing is fixed in advance and no point is left out."""
    from chicdiff_amd import hip
    rng = np.random.default_rng(1300 + S)
    a_pts = eval_points(S)
    K = len(a_pts)
    N = 64
    err = {}  # (quantity, decade) -> [gpu errors], [oracle errors]
    worst_alpha, worst_mu, npoints = 0.0, 0.0, 0
    for two_groups in (True, False):
        group = synth.groups(S) if two_groups else np.zeros(S, dtype=np.int32)
        kb, fb = design_rows(S, two_groups, rng)
        nb = len(kb)
        idx = np.arange(N) % nb
        counts, nf = kb[idx], fb[idx]
        dk, dn = ctx.to_device(counts, np.int32), ctx.to_device(nf, np.float64)
        A = np.tile(a_pts, (N, 1))
        dA = dev(ctx, A)
        prior_mean = -6.0 + 0.75 * (np.arange(N) % nb)
        prior_var = 0.7
        base = None
        for use_prior in (False, True):
            dpm = dev(ctx, prior_mean) if use_prior else None
            res = {}
            for live in [0] + sorted(LAYOUTS[S]):
                r = ctx.selftest_objective(dk, dn, group, dA, dpm, prior_var, live)
                assert r["lanes_per_row"] == (1 if live == 0 else LAYOUTS[S][live]), (S, live, r["lanes_per_row"])
                res[live] = {k: (v.cpu().numpy() if k != "lanes_per_row" else v) for k, v in r.items()}
            with pytest.raises(hip.ChicdiffHipError):  # the rule is not wider than the search's
                ctx.selftest_objective(dk, dn, group, dA, dpm, prior_var, TOO_MANY[S])
            g0 = res[0]
            assert np.isfinite(g0["lp"]).all() and np.isfinite(g0["dlp"]).all() and np.isfinite(g0["alpha"]).all()
            # every layout, and every copy of a base row (other lanes, other waves), returns the same bits
            for live, g in res.items():
                for q in ("lp", "dlp", "alpha", "mu"):
                    assert np.array_equal(bits(g[q]), bits(g0[q])), (S, two_groups, use_prior, live, q)
            for q in ("lp", "dlp", "alpha"):
                assert np.array_equal(bits(g0[q]), bits(g0[q][idx])), (S, two_groups, use_prior, q, "copies of a row differ")
            # mu = max(nf * group mean, minmu)
            mu = g0["mu"].T[:nb]  # (rows, S)
            qn = kb / fb
            gm = np.where(group[None, :] == 1, qn[:, group == 1].sum(axis=1, keepdims=True) / max(1, (group == 1).sum()),
                          qn[:, group == 0].sum(axis=1, keepdims=True) / (group == 0).sum())
            mu_np = np.maximum(fb * gm, 0.5)
            worst_mu = max(worst_mu, float(np.max(np.abs(mu - mu_np) / mu_np)))
            assert np.max(np.abs(mu - mu_np) / mu_np) <= 1e-13
            if two_groups:
                assert (mu[nb - 3 if S < 12 else nb - 2, S // 2:] == 0.5).all()  # the row whose group B is all zero sits at minmu
            # alpha = exp(a) to the documented 1 ulp
            ea = ulp_errors(g0["alpha"][0], [mp.exp(mp.mpf(float(v))) for v in a_pts])
            worst_alpha = max(worst_alpha, float(ea.max()))
            # the objective
            if base is None:
                base = [[mp_objective(a_pts[k], kb[i], mu[i], group, two_groups) for k in range(K)] for i in range(nb)]
            for i in range(nb):
                for k in range(K):
                    lp0, T0, dlp0, Td0 = base[i][k]
                    a = mp.mpf(float(a_pts[k]))
                    if use_prior:
                        dd = a - mp.mpf(float(prior_mean[i]))
                        pr, dpr = -dd * dd / (2 * mp.mpf(prior_var)), -dd / mp.mpf(prior_var)
                        lp0, T0, dlp0, Td0 = lp0 + pr, T0 + abs(pr), dlp0 + dpr, Td0 + abs(dpr)
                    kw = dict(prior_mean=float(prior_mean[i]), prior_sigmasq=prior_var, use_prior=use_prior)
                    o_lp = oracle.log_posterior(float(a_pts[k]), kb[i].astype(float), mu[i], group, **kw)
                    o_dlp = oracle.log_posterior(float(a_pts[k]), kb[i].astype(float), mu[i], group, deriv=True, **kw)
                    dec = int(math.floor(float(a_pts[k]) / math.log(10.0) + 1e-9))
                    for q, got, orc, ref, T in (("lp", g0["lp"][i, k], o_lp, lp0, T0), ("dlp", g0["dlp"][i, k], o_dlp, dlp0, Td0)):
                        e = err.setdefault((q, dec), ([], []))
                        e[0].append(float(abs(mp.mpf(float(got)) - ref) / (U * T)))
                        e[1].append(float(abs(mp.mpf(float(orc)) - ref) / (U * T)))
                    npoints += 1
    log_record("test_objective_against_50_digits", "mu vs max(nf * group mean, minmu), relative", f"S={S}", 4 * N * S, worst_mu, None, 1e-13)
    log_record("test_objective_against_50_digits", "alpha vs exp(a), ulp", f"S={S}", 4 * K, worst_alpha, None, 1.0)
    failed = []
    for (q, dec), (eg, eo) in sorted(err.items()):
        gw, ow = max(eg), max(eo)
        log_record("test_objective_against_50_digits", f"{q}, error in u*T", f"S={S} alpha in [1e{dec}, 1e{dec + 1})", len(eg), gw, ow, 4 * ow)
        if not gw <= 4 * ow:
            failed.append((q, dec, gw, ow))
    print(f"S={S}: {npoints} points (row, a, design, prior), each on {1 + len(LAYOUTS[S])} layouts")
    assert worst_alpha <= 1.0, worst_alpha
    assert not failed, failed


# ---------------------------------------------------------------------------------------------------------------------------
# 2. building blocks
# ---------------------------------------------------------------------------------------------------------------------------
def _r_points():
    r = list(np.exp(np.linspace(math.log(1.0 / 64), math.log(1e8), 41)))
    for k in range(10):
        c = float(10 - k)
        r += [np.nextafter(c, 0.0), c, np.nextafter(c, np.inf)]
    return r + [1.0 / 64, 1e8]


def _lgr_cases():
    xs, ys = [], []
    for r in _r_points():
        nr = int(math.ceil(10.0 - r)) if r < 10.0 else 0
        for y in sorted({0, 1, max(nr - 1, 0), nr, nr + 1, 1023, 1024, 10 ** 6, 2 ** 31 - 1}):
            xs.append(r)
            ys.append(y)
    return np.array(xs), np.array(ys, dtype=np.float64)


@pytest.mark.parametrize("op,name", [(10, "lgr_eval_t(lgr_make_t(r), y)"), (11, "lgr_eval(lgr_make(r), y)")])
def test_lgamma_difference(ctx, op, name):
    """lgamma(y + r) - lgamma(r) for r in [1/64, 1e8] (10 - k and both neighbours) and the counts at which the method changes.
    Unit: u (|ref| + 2 max(0, -log r)) — the sum of |log(r + i)|; allowance 4 units: the result is a sum of at most four same-signed
    terms, each a documented 1-ulp function times a once-rounded factor.  (A libm difference is no reference here: it loses
    5.8e-9 relative at r = 1e8.)"""
    x, y = _lgr_cases()
    got = ctx.selftest_math3(op, dev(ctx, x), dev(ctx, y))[0].cpu().numpy()
    worst, at = 0.0, None
    for r, yy, g in zip(x, y, got):
        rm = mp.mpf(float(r))
        ref = mp.loggamma(rm + int(yy)) - mp.loggamma(rm)
        unit = U * (abs(ref) + 2 * max(mp.mpf(0), -mp.log(rm)))
        e = 0.0 if (unit == 0 and g == 0.0) else (math.inf if unit == 0 else float(abs(mp.mpf(float(g)) - ref) / unit))
        if e > worst:
            worst, at = e, (float(r), int(yy), float(g))
    log_record("test_lgamma_difference", name + ", units of u (|ref| + 2 max(0, -log r))", "r in [1/64, 1e8]", len(x), worst, None, 4.0)
    assert worst <= 4.0, (worst, at)


def test_log_factorial(ctx):
    """log(y!) = lgr_eval(lgr_one(), y), and the host's table of it, which the kernels use below kLogFactN = 1024: both against
    loggamma(y + 1) to 4 units of u |ref|, and against each other to the same bound (the kernels switch between the two at 1024)."""
    y = np.array(sorted(set(range(0, 1100)) | {10 ** 6, 2 ** 31 - 1}), dtype=np.float64)
    x = np.ones_like(y)
    dev_y = dev(ctx, y)
    got = ctx.selftest_math3(12, dev(ctx, x), dev_y)[0].cpu().numpy()
    tab = ctx.selftest_math3(18, dev(ctx, x), dev_y)[0].cpu().numpy()
    ref = [mp.loggamma(mp.mpf(int(v)) + 1) for v in y]
    in_tab = y < 1024
    assert np.isnan(tab[~in_tab]).all() and np.isfinite(tab[in_tab]).all()
    e_fun = np.array([0.0 if (t == 0 and g == 0) else float(abs(mp.mpf(float(g)) - t) / (U * abs(t))) if t != 0 else math.inf
                      for g, t in zip(got, ref)])
    e_tab = np.array([0.0 if (t == 0 and g == 0) else float(abs(mp.mpf(float(g)) - t) / (U * abs(t))) if t != 0 else math.inf
                      for g, t in zip(tab[in_tab], ref)])
    with np.errstate(invalid="ignore", divide="ignore"):
        e_both = np.where(got[in_tab] == tab[in_tab], 0.0, np.abs(got[in_tab] - tab[in_tab]) / (U * np.abs(tab[in_tab])))
    log_record("test_log_factorial", "lgr_eval(lgr_one(), y) vs loggamma(y + 1), units of u |ref|", "y in 0..1099, 1e6, 2^31-1", len(y), e_fun.max(), None, 4.0)
    log_record("test_log_factorial", "host table vs loggamma(y + 1), units of u |ref|", "y < 1024", int(in_tab.sum()), e_tab.max(), None, 4.0)
    log_record("test_log_factorial", "lgr_eval(lgr_one(), y) vs host table, units of u |table|", "y < 1024", int(in_tab.sum()), e_both.max(), None, 4.0)
    assert e_fun.max() <= 4.0 and e_tab.max() <= 4.0 and e_both.max() <= 4.0, (e_fun.max(), e_tab.max(), e_both.max())


def _from_bits(b):
    return np.array(b, dtype=np.uint64).view(np.float64)


def _log_points():
    """Both edges of the 64 cells of tlog's table (the cell is the top six mantissa bits of bits(x) - 0x3FE6000000000000) in seven
    binades, 1 +- k ulp, and a random sample."""
    off = 0x3FE6000000000000
    pts = []
    for e in (-1000, -30, -1, 0, 1, 30, 1000):
        for i in range(64):
            b = off + (e << 52) + (i << 46)
            pts += [b - 2, b - 1, b, b + 1]
    x = list(_from_bits(pts))
    one = np.float64(1.0).view(np.uint64)
    x += list(_from_bits([int(one) + k for k in range(0, 65)] + [int(one) - k for k in range(1, 65)]))
    rng = np.random.default_rng(7)
    x += list(np.exp(rng.uniform(-700, 700, 1500))) + list(1 + rng.uniform(-0.05, 0.05, 500))
    return np.array(x, dtype=np.float64)


@pytest.mark.parametrize("op,name", [(0, "flog"), (1, "tlog")])
def test_log_is_within_one_ulp(ctx, op, name):
    """devmath.h: flog "<= 1 ulp"; tlog "<= 1.6 ulp, <= 2.6 ulp for x in [1 - 1/128, 1 + 1/64)".  tlog returns log c_i + r q.
    Outside the two cells with c = 1 the table's log c_i, rounded to half an ulp of ITS binade, can lie one binade above the result
    (|log x| just below a power of two: x = 0.8825, 0.939, 1.0645, ...) and then counts for a whole ulp; with the final rounding's half
    ulp and 0.1 for the product r q, the polynomial's own roundings and its truncation: 1.6.  In the cells with c = 1 the result is
    r q alone, and q ~ 1 is rounded twice at magnitude 1 (1 - r/2, then the last Estrin step): for x < 1 (q > 1, ulp 2^-52) each is
    up to one ulp of a result whose mantissa is near 1; with the product's half ulp and the same 0.1: 2.6 (x >= 1: q < 1, half of that).
    Measured in ulps of the true value at both edges of every table cell in seven binades, 1 +- k ulp, a random sample, and a dense
    sample of the cells around 1."""
    rng = np.random.default_rng(15)
    x = np.concatenate([_log_points(), rng.uniform(1 - 1.0 / 128, 1 + 1.0 / 64, 6000)])
    assert (x > 2.3e-308).all() and np.isfinite(x).all()
    got = ctx.selftest_math(op, dev(ctx, x)).cpu().numpy()
    e = ulp_errors(got, [mp.log(mp.mpf(float(v))) for v in x])
    near1 = (x >= 1 - 1.0 / 128) & (x < 1 + 1.0 / 64)
    b_out, b_in = (1.6, 2.6) if op == 1 else (1.0, 1.0)
    i, j = int(np.where(near1, 0, e).argmax()), int(np.where(near1, e, 0).argmax())
    log_record("test_log_is_within_one_ulp", name + ", ulp", "cell edges x 7 binades, random; outside [1 - 1/128, 1 + 1/64)", int((~near1).sum()), e[~near1].max(), None, b_out)
    log_record("test_log_is_within_one_ulp", name + ", ulp", "x in [1 - 1/128, 1 + 1/64): 1 +- k ulp, dense", int(near1.sum()), e[near1].max(), None, b_in)
    assert got[x == 1.0][0] == 0.0
    assert e[~near1].max() <= b_out, (name, e[i], float(x[i]).hex(), float(got[i]).hex())
    assert e[near1].max() <= b_in, (name, e[j], float(x[j]).hex(), float(got[j]).hex())


def test_rlog_guards(ctx):
    """rlog_t: the table logarithm strictly inside (2.3e-308, 1.7e308), the library's log outside — zero, negative, subnormal,
    huge, infinite and NaN arguments give what R's log() gives."""
    lo, hi = 2.3e-308, 1.7e308
    x = np.array([np.nextafter(lo, 0), lo, np.nextafter(lo, 1), np.nextafter(hi, 0), hi, np.nextafter(hi, np.inf), 2.2250738585072014e-308,
                  5e-324, 1e-310, 1.7976931348623157e308, 1.0, 0.0, -0.0, -1.0, np.inf, -np.inf, np.nan])
    got = ctx.selftest_math3(17, dev(ctx, x), dev(ctx, np.zeros_like(x)))[0].cpu().numpy()
    fin = np.isfinite(x) & (x > 0)
    e = ulp_errors(got[fin], [mp.log(mp.mpf(float(v))) for v in x[fin]])
    log_record("test_rlog_guards", "rlog_t, ulp", "both guards and their neighbours, subnormal, largest", int(fin.sum()), e.max(), None, 1.0)
    assert e.max() <= 1.0, e
    assert got[11] == -np.inf and got[12] == -np.inf and np.isnan(got[13]) and got[14] == np.inf and np.isnan(got[15]) and np.isnan(got[16])


def _exp_points():
    """Both sides of every boundary of texp's reduction (x = (k + 1/2) ln2 / 64: where rint() moves to the next table entry) and its
    centres (x = k ln2 / 64), all 64 entries in seven octaves of the result, +-700, 0, and the callers' range [-30, 10]."""
    c = mp.log(2) / 64
    x = []
    for m in (-1000, -40, -10, -1, 0, 1, 10, 14, 1000):
        for j in range(64):
            k = 64 * m + j
            for v in (float((k + mp.mpf(0.5)) * c), float(k * c)):
                x += [np.nextafter(np.nextafter(v, -np.inf), -np.inf), np.nextafter(v, -np.inf), v, np.nextafter(v, np.inf),
                      np.nextafter(np.nextafter(v, np.inf), np.inf)]
    rng = np.random.default_rng(8)
    x += [700.0, -700.0, 0.0, -0.0, -30.0, 10.0] + list(rng.uniform(-30, 10, 3000)) + list(rng.uniform(-1e-3, 1e-3, 300))
    return np.array(x, dtype=np.float64)


def test_exp_is_within_one_ulp(ctx):
    """devmath.h: texp "<= 1 ulp"."""
    x = _exp_points()
    got = ctx.selftest_math(8, dev(ctx, x)).cpu().numpy()
    e = ulp_errors(got, [mp.exp(mp.mpf(float(v))) for v in x])
    i = int(e.argmax())
    log_record("test_exp_is_within_one_ulp", "texp, ulp", "reduction boundaries and centres x 9 octaves, +-700, [-30, 10]", len(x), e.max(), None, 1.0)
    assert (got[x == 0.0] == 1.0).all()
    assert e.max() <= 1.0, (e.max(), float(x[i]).hex(), float(got[i]).hex())


def test_rcp_is_within_one_ulp(ctx):
    """devmath.h: rcp "< 1 ulp" — near powers of two, where the result changes binade, and on a random sample."""
    pts = []
    for e in (-500, -1, 0, 1, 500):
        b = int(np.float64(2.0 ** e).view(np.uint64))
        pts += [b + k for k in range(-32, 33)]
    rng = np.random.default_rng(9)
    x = np.concatenate([_from_bits(pts), np.exp(rng.uniform(-600, 600, 2000)), rng.uniform(1, 2, 1000)])
    got = ctx.selftest_math(2, dev(ctx, x)).cpu().numpy()
    e = ulp_errors(got, [1 / mp.mpf(float(v)) for v in x])
    i = int(e.argmax())
    log_record("test_rcp_is_within_one_ulp", "rcp, ulp", "2^e +- 32 ulp (e = -500, -1, 0, 1, 500), random", len(x), e.max(), None, 1.0)
    assert e.max() < 1.0, (e.max(), float(x[i]).hex(), float(got[i]).hex())


def test_rcp_or_div(ctx):
    """rcp_or_div: rcp() (< 1 ulp) strictly inside (1e-300, 1e300), the IEEE division — the correctly rounded quotient, signed zeros,
    infinities, NaN — everywhere else."""
    edge = [1e-300, np.nextafter(1e-300, 1), np.nextafter(1e-300, 0), 1e300, np.nextafter(1e300, 0), np.nextafter(1e300, np.inf)]
    other = [0.0, -0.0, 5e-324, 1e-310, 2.2250738585072014e-308, 1.7976931348623157e308, np.inf, -np.inf, np.nan, -1.0, -3.0, -1e-305, -1e305, 1e-305, 1e305]
    rng = np.random.default_rng(10)
    x = np.array(edge + other + list(np.exp(rng.uniform(-690, 690, 1000))))
    got = ctx.selftest_math3(15, dev(ctx, x), dev(ctx, np.zeros_like(x)))[0].cpu().numpy()
    inside = (x > 1e-300) & (x < 1e300)
    e = ulp_errors(got[inside], [1 / mp.mpf(float(v)) for v in x[inside]])
    log_record("test_rcp_or_div", "rcp_or_div inside (1e-300, 1e300), ulp", "guards' neighbours, random", int(inside.sum()), e.max(), None, 1.0)
    assert e.max() < 1.0
    with np.errstate(divide="ignore", invalid="ignore"):
        want = 1.0 / x[~inside]
    same = (bits(got[~inside]) == bits(want)) | (np.isnan(got[~inside]) & np.isnan(want))
    log_record("test_rcp_or_div", "rcp_or_div outside: results that differ from the IEEE quotient", "zero, subnormal, huge, infinite, NaN, negative", int((~inside).sum()), float((~same).sum()), None, 0.0)
    assert same.all(), (x[~inside][~same], got[~inside][~same], want[~same])


@pytest.mark.parametrize("op,name,bound", [(13, "tlog1p_from", 2.1), (14, "flog1p_from", 1.5)])
def test_log1p_forms(ctx, op, name, bound):
    """log1p(u) = log(t) + (u - (t - 1)) / t with t = 1 + u rounded, as the objective (u = mu alpha) and lgr_eval (u = d / z0) call it.
    Bound: the logarithm's documented error for an argument t >= 1 (flog 1 ulp, tlog 1.6 ulp) plus half an ulp for the final
    fma; the correction term's own errors (the 1-ulp reciprocal, the dropped second-order term delta^2 / 2 t^2 with
    delta <= 2^-53 t) are below 2^-100 relative."""
    rng = np.random.default_rng(11)
    u = np.concatenate([np.exp(rng.uniform(math.log(1e-18), math.log(1e14), 3000)), [0.0, 2.0 ** -53, 2.0 ** -52, 1e-16, 0.5, 1.0, 3.0, 1e14],
                        2.0 ** -np.arange(1, 60.0), 1 - 2.0 ** -np.arange(1, 53.0), rng.uniform(0, 1.0 / 64, 2000)])
    got = ctx.selftest_math3(op, dev(ctx, u), dev(ctx, np.zeros_like(u)))[0].cpu().numpy()
    e = ulp_errors(got, [mp.log1p(mp.mpf(float(v))) for v in u])
    i = int(e.argmax())
    log_record("test_log1p_forms", name + "(u, 1 + u, rcp(1 + u)), ulp", "u in [1e-18, 1e14], [0, 1/64), powers of two, 0", len(u), e.max(), None, bound)
    assert e.max() <= bound, (e.max(), float(u[i]).hex(), float(got[i]).hex())


def test_stirling(ctx):
    """stirling(z, tlog(z), rcp(z)) for z >= 10: lgamma(z) in units of u (|(z - 1/2) log z| + z + log sqrt(2 pi)) and digamma(z) in units
    of u (log z + 1 / 2z) — the terms before cancellation —, 4 units each: three 1-ulp inputs (log, reciprocal, the series) times
    once-rounded factors, summed with two or three roundings; the series' truncation (< 4e-17 / 5e-17 absolute) is under 0.1 unit."""
    rng = np.random.default_rng(12)
    z = np.concatenate([[10.0, np.nextafter(10.0, 11), 10.5, 11.0, 19.0, 1e8, 1e8 + 2 ** 31 - 1, 2.0 ** 31 + 9, 1e13],
                        10 + rng.uniform(0, 1, 500), np.exp(rng.uniform(math.log(10), math.log(2e13), 2000))])
    lg, dg = (t.cpu().numpy() for t in ctx.selftest_math3(16, dev(ctx, z), dev(ctx, np.zeros_like(z))))
    e_lg = np.empty(len(z))
    e_dg = np.empty(len(z))
    for i, v in enumerate(z):
        zm = mp.mpf(float(v))
        ul = U * (abs((zm - mp.mpf(0.5)) * mp.log(zm)) + zm + mp.log(mp.sqrt(2 * mp.pi)))
        ud = U * (mp.log(zm) + 1 / (2 * zm))
        e_lg[i] = float(abs(mp.mpf(float(lg[i])) - mp.loggamma(zm)) / ul)
        e_dg[i] = float(abs(mp.mpf(float(dg[i])) - mp.digamma(zm)) / ud)
    log_record("test_stirling", "stirling lg vs loggamma, units of u (|(z - 1/2) log z| + z + 0.92)", "z in [10, 2e13]", len(z), e_lg.max(), None, 4.0)
    log_record("test_stirling", "stirling dg vs digamma, units of u (log z + 1 / 2z)", "z in [10, 2e13]", len(z), e_dg.max(), None, 4.0)
    assert e_lg.max() <= 4.0 and e_dg.max() <= 4.0, (e_lg.max(), float(z[e_lg.argmax()]), e_dg.max(), float(z[e_dg.argmax()]))


def test_pnorm_whole_domain(ctx, oracle):
    """2 pnorm(-|z|) against erfc(|z| / sqrt 2), segment by segment of Cody's algorithm; bound per segment: 4 x the oracle's worst
    relative error on the same points in the same run.  Exact values must be equal.  (The function has no results in the subnormal
    range: below the cutoff 37.5193 the smallest is 4.46e-308, from there on it is 0 — asserted below.)"""
    b1, b2, b3 = 0.67448975, 5.656854249492380195206754896838, 37.5193
    rng = np.random.default_rng(13)

    def around(v, k=3):
        out = [v]
        lo = hi = v
        for _ in range(k):
            lo, hi = np.nextafter(lo, -np.inf), np.nextafter(hi, np.inf)
            out += [lo, hi]
        return out

    z = np.concatenate([rng.uniform(0, b1, 600), rng.uniform(b1, b2, 900), rng.uniform(b2, b3, 900), rng.uniform(b3, 45, 50),
                        rng.uniform(36.5, b3, 300),  # results between 1e-291 and the smallest normal number
                        around(b1), around(b2), around(b3), around(1.1102230246251565e-16), [1e-17, 5e-324, 1e-300, 38.0, 40.0, 1e10]])
    z = np.concatenate([z, -z])
    got = ctx.selftest_math(5, dev(ctx, z)).cpu().numpy()
    orc = oracle.pnorm_two_sided(z)
    y = np.abs(z)
    seg = np.where(y <= b1, 0, np.where(y <= b2, 1, np.where(y < b3, 2, 3)))
    names = ["|z| <= 0.67448975", "0.67448975 < |z| <= sqrt 32", "sqrt 32 < |z| < 37.5193", "|z| >= 37.5193 (the result is 0 by definition)"]
    ref = [mp.erfc(mp.mpf(float(v)) / mp.sqrt(2)) for v in y]
    eg = np.array([float(abs(mp.mpf(float(g)) - t) / (U * t)) for g, t in zip(got, ref)])
    eo = np.array([float(abs(mp.mpf(float(g)) - t) / (U * t)) for g, t in zip(orc, ref)])
    failed = []
    for s in range(4):
        m = seg == s
        log_record("test_pnorm_whole_domain", "pnorm_two_sided, relative error in u", names[s], int(m.sum()), eg[m].max(), eo[m].max(), 4 * eo[m].max())
        if not eg[m].max() <= 4 * eo[m].max():
            failed.append((names[s], eg[m].max(), eo[m].max()))
    assert (got[seg == 3] == 0.0).all() and (got[seg != 3] >= 2.2250738585072014e-308).all()
    special = np.array([0.0, -0.0, np.inf, -np.inf, np.nan])
    gs = ctx.selftest_math(5, dev(ctx, special)).cpu().numpy()
    assert gs[0] == 1.0 and gs[1] == 1.0 and gs[2] == 0.0 and gs[3] == 0.0 and np.isnan(gs[4])
    assert not failed, failed


# ---------------------------------------------------------------------------------------------------------------------------
# 3. the reported deviance against the fit's own parameters
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("two_groups,prior_var", [(True, None), (False, None), (True, 1e6)], ids=["condition", "intercept", "condition-wide-prior"])
def test_deviance_from_own_parameters(ctx, two_groups, prior_var):
    """deviance = -2 sum_j log dnbinom(y_j; size = 1 / alpha, mu_j = nf_j 2^eta_j), rebuilt in mpmath from the dispersion, intercept and
    log2FoldChange the GPU itself reports (rows whose coefficients come from the converged IRLS, and every row of a ~1 fit).
    Unit: u (sum_j |lgamma(y + size) - lgamma(size)| + |log y!| + |y log(alpha mu)| + |(size + y) log1p(alpha mu)|) plus the first-order
    effect of eta's own rounding, u |sum_j (y - mu) / (1 + alpha mu)| max(1, |eta|); allowance 4 units, as for the lgamma difference.
    sumDeviance: the exactly rounded sum of the rows' values, to n u relative.
    Under the fitted prior no final dispersion reaches minDisp (the prior pulls an underdispersed row to the trend); the third case
    fits with a flat prior (dispPriorVar = 1e6), where such rows end at minDisp exactly, and requires some in the sample.  A single
    count of 16 000 or more among means of ~20 takes a ~condition row off the IRLS path (100 iterations, then the optimiser): the
    planted counts run from 2 000 to 2 048 000, and the sample must hold some of them in either design."""
    S, n0 = 8, 6000
    d = synth.make(n0, S)
    rng = np.random.default_rng(14)
    counts, nf = d["counts"].copy(), d["nf"].copy()
    for i in range(40):  # underdispersed rows (they end at alpha = minDisp) and rows with one huge count
        counts[i] = np.rint(nf[i] * (20.0 + 40.0 * i))
        counts[100 + i, rng.integers(0, S)] = 2000 * 2 ** (i % 11)
    keep = counts.sum(axis=1) > 0
    counts, nf = counts[keep], nf[keep]
    group = synth.groups(S) if two_groups else np.zeros(S, dtype=np.int32)
    got, sc = tgp.run_fit(ctx, dict(counts=counts, nf=nf), group, **(dict(dispPriorVar=prior_var) if prior_var else {}))
    n = len(counts)
    assert (got["allZero"] == 0).all()
    ok = (got["betaConv"] == 1) & (got["betaIter"] < 100) & np.isfinite(got["deviance"]) if two_groups else np.isfinite(got["deviance"])
    if not two_groups:
        assert ok.all()
    at_floor = np.flatnonzero(ok & (got["dispersion"] <= 1e-8))
    huge = np.flatnonzero(ok & (counts.max(axis=1) >= 2000) & (np.arange(n) < 200))
    assert len(huge) > 0 and (len(at_floor) > 0 or not prior_var), (len(at_floor), len(huge))
    rows = np.unique(np.concatenate([at_floor, huge, rng.choice(np.flatnonzero(ok), 1200, replace=False)]))
    worst, at = 0.0, None
    for i in rows:
        al = mp.mpf(float(got["dispersion"][i]))
        size = 1 / al
        lg_s = mp.loggamma(size)
        b0 = mp.mpf(float(got["intercept"][i]))
        b1 = mp.mpf(float(got["log2FoldChange"][i])) if two_groups else mp.mpf(0)
        ll = T = sens = mp.mpf(0)
        eta_max = mp.mpf(1)
        for j in range(S):
            eta = b0 + b1 * int(group[j])
            eta_max = max(eta_max, abs(eta))
            mu = mp.mpf(float(nf[i, j])) * mp.power(2, eta)
            y = mp.mpf(int(counts[i, j]))
            am = al * mu
            t1 = mp.loggamma(y + size) - lg_s
            t2 = mp.loggamma(y + 1)
            t3 = y * mp.log(am) if y else mp.mpf(0)
            t4 = (size + y) * mp.log1p(am)
            ll += t1 - t2 + t3 - t4
            T += abs(t1) + abs(t2) + abs(t3) + abs(t4)
            sens += (y - mu) / (1 + am)
        unit = 2 * U * (T + abs(sens) * eta_max)
        e = float(abs(mp.mpf(float(got["deviance"][i])) - (-2 * ll)) / unit)
        if e > worst:
            worst, at = e, int(i)
    tag = ("~condition" if two_groups else "~1") + (f", dispPriorVar = {prior_var:g}" if prior_var else "")
    log_record("test_deviance_from_own_parameters", "deviance vs -2 sum log dnbinom at the reported parameters, units (docstring)",
               f"{tag}, {n} x {S}: rows at minDisp ({len(at_floor)}), one huge count ({len(huge)}), random", len(rows), worst, None, 4.0)
    exact = math.fsum(float(v) for v in got["deviance"])
    rel = abs(sc["sumDeviance"] - exact) / abs(exact)
    log_record("test_deviance_from_own_parameters", "sumDeviance vs the exactly rounded sum of the rows, relative", f"{tag}, {n} rows", n, rel, None, n * U)
    assert worst <= 4.0, (worst, at, counts[at], float(got["dispersion"][at]))
    assert rel <= n * U, (rel, sc["sumDeviance"], exact)
