"""The theta scan (chicdiff_hip_theta_grid_dev) and the route its fits take, against the twins.

With more than one theta in flight every fit of the scan runs on a child context whose trend is one launch per IRLS pass
(trend_pass_kernel<<<512, 256>>> + trend_reduce_kernel with the fused step), followed by resid_kernel, two selects and
prior_var_kernel or prior_mc — the route of any context after a grid-barrier timeout, and of the options trend_one_launch_per_pass = 1
and trend_mad_in_kernel = 0.  Every other twin test runs the default route (trend_persistent_kernel with the median and the MAD in the
same launch).  Here:

  a  five free fits (disp_inputs.FREE_FITS, and design ~1 at S = 4 and S = 8) by the default route and under each of the two options:
     status bits, trend coefficients, trendOuterIter, dispFit, varLogDispEsts and the prior variance (closed form, or matched by
     simulation: exactly) under test_disp_twin.judge_global on the device's own baseMean and dispGeneEst, within ALLOWANCE x
     max(the oracle's routines on the same columns, FLOOR) — the form and the constants of tests/test_gpu_disp.py; everything upstream
     of the trend by bits; under trend_mad_in_kernel = 0 the trend itself by bits;
  b  the cases trend-edges of tests/theta_inputs.py through chicdiff_hip_selftest_global_stage_dev (which calls cd::global_stage, so
     the option applies) under trend_one_launch_per_pass = 1, and by the default route beside it: the same judge; the NaN pattern of the
     residual column against the rule of resid_kernel and every finite residual against its row formula on the reported coefficients;
     the 262 961-row tiling of the 599 rows, where trend_pass_kernel's grid-stride loop wraps, against the twin of the 599 rows.  (The
     entry leaves dispFit NaN under a parametric trend — the column is written by the MAP launch, disp_kernels.hip, which the entry does
     not run — so the per-row check of this stage is on `resid`, the column it does write, and dispFit is required to be NaN.)
  c  every total of a grid with 2, 5 or 16 fits in flight is, bit for bit, the sumDeviance of the single fit on a second context with
     trend_one_launch_per_pass = 1 (both take the same branch of global_stage: the fixed 512-block partition, the fixed-order reduction,
     the separate MAD; the offsets formed inside prep are offsets_kernel's by bits, tests/test_prep_offsets_classes_gpu.py); with one fit
     in flight the grid runs on the parent and returns the bits of the default single fit.  Lane plans of 1 .. 11 thetas on 1 .. 16
     lanes, equal thetas, a permuted grid, workspaces reused across shapes; after every grid call a default fit on the parent has its
     earlier bits; the oracle's argmin (gap >= 1e-6, tests/test_theta_inputs.py) and 1e-7 per theta at every lane count.
  d  sumDeviance against math.fsum of the fit's own reported deviance column (wald_intercept_kernel adds exactly the value it reports,
     dev_sum_kernel the 3072 block partials: nothing had to be rebuilt) within (n - 1) 2^-53 sum |deviance_i|, the bound of any
     summation order; an all-zero row makes every total NaN (sum() without na.rm), and the mirror raises.

Every comparison goes to test_gpu_parity.PARITY_LOG (profiles/r63_theta_scan_accuracy.json holds the records of one run).
"""
import contextlib
import math

import mpmath as mp
import numpy as np
import pytest

import disp_inputs as di
import disp_twin as dt
import test_disp_twin as td
import test_gpu_disp as tgd
import test_gpu_parity as tgp
import test_theta_inputs as tti
import theta_inputs as th
from test_gpu_disp import ALLOWANCE, FLOOR
from test_gpu_objective import log_record

pytestmark = pytest.mark.gpu

ST_FAILED, ST_MC, ST_LOCAL = 1, 2, 16
DEFAULTS = {"trend_one_launch_per_pass": 0, "trend_mad_in_kernel": 1, "theta_grid_concurrency": 5}
ROUTES = {"default": {}, "trend_one_launch_per_pass=1": {"trend_one_launch_per_pass": 1}, "trend_mad_in_kernel=0": {"trend_mad_in_kernel": 0}}
UPSTREAM = ["baseMean", "baseVar", "dispGeneEst", "dispGeneIter", "allZero"]
LANES = (2, 5, 16)
POOL = [0.0, 1.0, 0.5, 0.25, 0.75, 0.1, 0.9, 0.33, 0.66, 0.05, 0.95]  # the thetas of the lane plans: its first ntheta
GRID_CASES = list(th.SCANS) + ["scan-na"]


@pytest.fixture(scope="module")
def ctx():
    import __graft_entry__ as g
    g.build()  # no-op when the in-tree library and the oracle are up to date
    from chicdiff_amd import hip
    c = hip.HipContext(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def ctx2(ctx):
    """A second context whose single fits take the lanes' route."""
    from chicdiff_amd import hip
    c = hip.HipContext(0)
    c.set_option("trend_one_launch_per_pass", 1)
    yield c
    c.close()


@pytest.fixture(scope="module")
def oracle():
    from oracle import oracle as o
    return o


@contextlib.contextmanager
def options(c, **kw):
    try:
        for k, v in kw.items():
            c.set_option(k, v)
        yield
    finally:
        for k in kw:
            c.set_option(k, DEFAULTS[k])


def differ(a, b):
    """How many elements of two columns differ by bits (NaN equals NaN)."""
    a, b = np.asarray(a), np.asarray(b)
    if a.dtype.kind != "f":
        return int(np.sum(a != b))
    return int(np.sum(~td.same_bits(a, b)))


def within(test, name, dev, ora):
    """Every quantity of the device within ALLOWANCE x max(yardstick, FLOOR); logs each.  Returns what fails."""
    failed = []
    for q, e in sorted(dev.items()):
        allowed = ALLOWANCE * max(ora[q], FLOOR)
        log_record(test, f"{q}, units of tests/disp_twin.py", name, 1, e, ora[q], allowed)
        if not e <= allowed:
            failed.append((q, e, ora[q]))
    return failed


# ---------------------------------------------------------------------------------------------------------------------------
# a. the product path by three routes
# ---------------------------------------------------------------------------------------------------------------------------
A_CASES = {name: (name, False) for name in di.FREE_FITS}
A_CASES.update({"1500x4~1": ("1500x4", True), "2051x8~1": ("2051x8", True)})


def a_fit(name):
    base, intercept_only = A_CASES[name]
    fit = dict(di.make_free(base), name=name)
    if intercept_only:
        fit["group"] = np.zeros(fit["S"], dtype=np.int32)
    return fit


ROUTE_FINDINGS = {}  # {(case, route): dict(trendCoef, varLogDispEsts, dispPriorVar: equal to the default route's by bits?)}


@pytest.mark.parametrize("name", list(A_CASES))
def test_fit_routes_against_twin(ctx, oracle, name):
    """One free fit by the default route, with the trend as one launch per pass, and with the MAD outside the trend kernel."""
    t = "test_fit_routes_against_twin"
    fit = a_fit(name)
    S = fit["S"]
    p = 2 if fit["group"].any() else 1
    got = {}
    for route, opt in ROUTES.items():
        with options(ctx, **opt):
            got[route] = tgd.device_fit(ctx, fit["counts"], fit["nf"], fit["group"], None)
    base = got["default"]
    for route in list(ROUTES)[1:]:
        off = {k: differ(got[route][k], base[k]) for k in UPSTREAM}
        log_record(t, "values upstream of the trend that differ from the default route's by bits", f"{name} | {route}", len(UPSTREAM) * len(base["baseMean"]),
                   sum(off.values()), None, 0)
        assert not any(off.values()), (name, route, off)
    with mp.workdps(dt.DPS):
        twin = dt.global_stage(base["baseMean"], base["dispGeneEst"], S, p)
    fitted, ysc, _ = tti.yardstick(oracle, base["baseMean"], base["dispGeneEst"], base["allZero"], S, p)
    ora = td.judge_global(fit, dict(base, dispFit=fitted), ysc, twin=twin)
    assert not ora["violations"], ("the yardstick itself", ora["violations"])
    for route, g in got.items():
        stratum = f"{name} | {route}"
        want_status = ST_MC if S - p <= 3 else 0
        assert g["status"] & (ST_FAILED | ST_LOCAL | ST_MC) == want_status, (stratum, g["status"])
        dev = td.judge_global(fit, g, g, twin=twin)
        log_record(t, "violations: trendOuterIter, argmin of the simulated prior", stratum, 1, len(dev["violations"]), len(ora["violations"]), 0)
        log_record(t, "decisions excused as near", stratum, 1, dev["near"], ora["near"], 1)
        assert not dev["violations"], (stratum, dev["violations"])
        assert "dispPriorVar" in dev["errors"] and "dispFit" in dev["errors"]
        failed = within(t, stratum, dev["errors"], ora["errors"])
        assert not failed, (stratum, failed)
        if route != "default":
            same = {k: differ(np.atleast_1d(g[k]), np.atleast_1d(base[k])) == 0 for k in ("trendCoef", "varLogDispEsts", "dispPriorVar", "trendOuterIter")}
            ROUTE_FINDINGS[(name, route)] = same
            for k, v in same.items():  # a finding, recorded either way (the documentation of the options follows it)
                log_record(t, f"{k} differs from the default route's by bits (1 = yes)", stratum, 1, 0 if v else 1, None, 1)
            print(f"{stratum}: equal to the default route by bits: {same}")
    # the MAD outside the kernel leaves the trend to the persistent kernel
    assert ROUTE_FINDINGS[(name, "trend_mad_in_kernel=0")]["trendCoef"] and ROUTE_FINDINGS[(name, "trend_mad_in_kernel=0")]["trendOuterIter"], ROUTE_FINDINGS


# ---------------------------------------------------------------------------------------------------------------------------
# b. the kernel edges through the global-stage entry
# ---------------------------------------------------------------------------------------------------------------------------
def stage_outputs(ctx, case):
    from chicdiff_amd import hip
    d = [ctx.to_device(np.ascontiguousarray(case[k]), ty) for k, ty in (("baseMean", np.float64), ("dispGeneEst", np.float64), ("allZero", np.int32))]
    r = ctx.selftest_global_stage(d[0], d[1], d[2], case["S"], case["p"], hip.default_opts(**case["opts"]))
    return dict(scalars=r["scalars"], dispFit=r["dispFit"].cpu().numpy(), resid=r["resid"].cpu().numpy())


_YARD = {}


def stage_yardstick(oracle, case):
    if case["name"] not in _YARD:
        fitted, sc, resid = tti.yardstick(oracle, case["baseMean"], case["dispGeneEst"], case["allZero"], case["S"], case["p"])
        rows = judged_rows(case)
        wrong, worst = tti.judge_resid(case["baseMean"], case["dispGeneEst"], case["allZero"], sc["trendCoef"], resid, rows)
        _YARD[case["name"]] = (tti.judge_stage(case, sc), wrong, worst)
    return _YARD[case["name"]]


def judged_rows(case):
    """The rows whose residual goes through 50-digit arithmetic: all, or the first and the last copy of the tiled case (the copies
    between are compared with the first by bits)."""
    n = len(case["baseMean"])
    return range(n) if "copies" not in case else list(range(599)) + list(range(n - 599, n))


@pytest.mark.parametrize("route", ["trend_one_launch_per_pass=1", "default"])
@pytest.mark.parametrize("name", th.EDGES)
def test_stage_edges_against_twin(ctx, oracle, name, route):
    t = "test_stage_edges_against_twin"
    case = th.edge_case(name)
    stratum = f"{name} | {route}"
    with options(ctx, **ROUTES[route]):
        out = stage_outputs(ctx, case)
    sc = out["scalars"]
    n = len(case["baseMean"])
    want_status = ST_MC if case["S"] - case["p"] <= 3 else 0
    assert sc["status"] & (ST_FAILED | ST_LOCAL | ST_MC) == want_status, (stratum, sc["status"])
    dev = tti.judge_stage(case, sc)
    ora, ora_wrong, ora_resid = stage_yardstick(oracle, case)
    log_record(t, "violations: trendOuterIter, argmin of the simulated prior", stratum, 1, len(dev["violations"]), len(ora["violations"]), 0)
    log_record(t, "decisions excused as near", stratum, 1, dev["near"], ora["near"], 0)
    assert not ora["violations"] and ora["near"] == 0 and not ora_wrong, ("the yardstick itself", ora["violations"], ora_wrong)
    assert not dev["violations"] and dev["near"] == 0, (stratum, dev["violations"])  # (no decision of these cases is near: tests/test_theta_inputs.py)
    failed = within(t, stratum, dev["errors"], ora["errors"])
    # the residual column: the rule of resid_kernel, and the row formula on the reported coefficients
    rows = judged_rows(case)
    wrong, worst = tti.judge_resid(case["baseMean"], case["dispGeneEst"], case["allZero"], sc["trendCoef"], out["resid"], rows)
    log_record(t, "rows whose residual is NaN against the rule, or not finite", stratum, len(rows), len(wrong), len(ora_wrong), 0)
    allowed = ALLOWANCE * max(ora_resid, FLOOR)
    log_record(t, "resid, units of tests/trend_twin.residuals", stratum, len(rows), worst, ora_resid, allowed)
    assert not wrong, (stratum, wrong[:10])
    pl = case["planted"]
    first = out["resid"][:599] if "copies" in case else out["resid"]
    assert np.isnan(first[pl["zero"]]).all() and np.isnan(first[pl["below"]]).all() and np.isfinite(first[pl["at"]]).all() and np.isfinite(first[pl["above"]]).all()
    if not worst <= allowed:
        failed.append(("resid", worst, ora_resid))
    assert not failed, (stratum, failed)
    # a parametric trend's dispFit is the MAP launch's to write: this entry leaves the column NaN
    assert np.isnan(out["dispFit"]).all(), stratum
    if "copies" in case:
        K = case["copies"]
        off = {k: int(np.sum(~td.same_bits(out[k].reshape(K, 599), np.broadcast_to(out[k][:599], (K, 599))))) for k in ("resid", "dispFit")}
        log_record(t, "values of resid and dispFit that differ from the first copy's by bits", stratum, 2 * n, sum(off.values()), None, 0)
        assert not any(off.values()), (stratum, off)


# ---------------------------------------------------------------------------------------------------------------------------
# c. every fit of the grid is the single fit
# ---------------------------------------------------------------------------------------------------------------------------
_DEVICE, _SINGLE, _SENTINEL = {}, {}, {}


def on_device(c, case):
    key = (id(c), case["name"])
    if key not in _DEVICE:
        _DEVICE[key] = (c.to_device(case["counts"], np.int32), c.to_device(case["FullMean"], np.float64))
    return _DEVICE[key]


def single(c, case, theta, want=("deviance",)):
    """The design-~1 single fit of one theta on context c: (sumDeviance, scalars, columns); sumDeviance cached per (context, case, theta)."""
    dk, dF = on_device(c, case)
    S = case["counts"].shape[1]
    out, sc = c.nbglm_fit(dk, c.offsets(dF, case["sf"], theta), np.zeros(S, dtype=np.int32), want=list(want))
    return sc["sumDeviance"], sc, {k: v.cpu().numpy() for k, v in out.items()}


def single_total(c, case, theta):
    key = (id(c), case["name"], float(theta))
    if key not in _SINGLE:
        _SINGLE[key] = single(c, case, theta)[0]
    return _SINGLE[key]


def grid(ctx, case, thetas, lanes):
    """ctx.theta_grid with `lanes` fits in flight; afterwards a default fit on the parent must have the bits it had before any grid call
    of this session (the lanes touch neither the parent's options nor its workspace)."""
    dk, dF = on_device(ctx, case)
    with options(ctx, theta_grid_concurrency=lanes):
        g = ctx.theta_grid(dk, dF, case["sf"], list(thetas))
    total, _, cols = single(ctx, case, 0.5)
    t0, d0 = _SENTINEL[case["name"]]
    off = differ([total], [t0]) + differ(cols["deviance"], d0)
    log_record("grid", "values of a default fit on the parent after the grid call that differ from before it", f"{case['name']} | {len(thetas)} thetas, {lanes} lanes",
               1 + len(d0), off, None, 0)
    assert off == 0, (case["name"], lanes, total, t0)
    return g


def assert_grid_is_single(test, c_ref, case, thetas, g, lanes, route):
    ref = np.array([single_total(c_ref, case, t) for t in thetas])
    bad = [f"theta = {t}, {lanes} lanes: grid {a!r}, single fit ({route}) {b!r}" for t, a, b in zip(thetas, g, ref) if differ([a], [b])]
    log_record(test, f"totals that differ by bits from the single fit ({route})", f"{case['name']} | {len(thetas)} thetas, {lanes} lanes", len(thetas), len(bad), None, 0)
    assert np.isfinite(g).all() and not bad, bad


def prime(ctx, ctx2, case, thetas):
    """The single fits of both routes, and the default fit that every grid call is followed by, before any grid call on this case."""
    if case["name"] not in _SENTINEL:
        total, _, cols = single(ctx, case, 0.5)
        _SENTINEL[case["name"]] = (total, cols["deviance"])
    for t in thetas:
        single_total(ctx, case, t)
        single_total(ctx2, case, t)


@pytest.mark.parametrize("name", GRID_CASES)
def test_grid_totals_are_the_single_fits(ctx, ctx2, oracle, name):
    """2, 5 and 16 fits in flight: the per-pass single fit's bits; one fit in flight and one-point grids: the default single fit's; the
    oracle's argmin and 1e-7 per theta at every lane count."""
    t = "test_grid_totals_are_the_single_fits"
    case = th.scan_case(name)
    thetas = case["thetas"]
    prime(ctx, ctx2, case, thetas)
    ref = tti.oracle_deviances(oracle, name)
    for lanes in (1,) + LANES:
        g = grid(ctx, case, thetas, lanes)
        if lanes == 1:
            assert_grid_is_single(t, ctx, case, thetas, g, lanes, "default route")
        else:
            assert_grid_is_single(t, ctx2, case, thetas, g, lanes, "trend_one_launch_per_pass = 1")
        r = np.abs(g - ref) / np.abs(ref)
        log_record(t, "total deviance against the oracle, relative", f"{name} | {lanes} lanes", len(thetas), r.max(), None, 1e-7)
        assert np.allclose(g, ref, rtol=1e-7), (lanes, g, ref)
        assert np.argmin(g) == np.argmin(ref), (lanes, g, ref)
    for lanes in (5, 16):  # a one-point grid runs on the parent at any setting
        for th1 in thetas:
            g = grid(ctx, case, [th1], lanes)
            assert_grid_is_single(t, ctx, case, [th1], g, lanes, "default route")


@pytest.mark.parametrize("lanes", (1, 2, 5, 16))
@pytest.mark.parametrize("ntheta", (1, 2, 5, 7, 11))
def test_lane_plans(ctx, ctx2, ntheta, lanes):
    """ntheta thetas on min(ntheta, lanes) lanes (lane k fits the points k, k + lanes, ...): each total is its single fit."""
    case = th.scan_case("scan-S8")
    prime(ctx, ctx2, case, POOL)
    thetas = POOL[:ntheta]
    g = grid(ctx, case, thetas, lanes)
    on_parent = min(ntheta, lanes) == 1
    assert_grid_is_single("test_lane_plans", ctx if on_parent else ctx2, case, thetas, g, lanes, "default route" if on_parent else "trend_one_launch_per_pass = 1")


def test_equal_and_permuted_thetas(ctx, ctx2):
    """Seven equal thetas on five lanes give seven identical doubles (no lane reads another's workspace); a permuted grid gives the
    permuted doubles (lane k then fits other points)."""
    t = "test_equal_and_permuted_thetas"
    case = th.scan_case("scan-S8")
    prime(ctx, ctx2, case, POOL)
    g = grid(ctx, case, [0.25] * 7, 5)
    assert_grid_is_single(t, ctx2, case, [0.25] * 7, g, 5, "trend_one_launch_per_pass = 1")
    assert len(set(g.tolist())) == 1, g
    thetas = POOL[:7]
    perm = [3, 6, 0, 5, 1, 4, 2]
    a, b = grid(ctx, case, thetas, 5), grid(ctx, case, [thetas[i] for i in perm], 5)
    log_record(t, "totals of a permuted grid that differ from the permuted totals", "scan-S8 | 7 thetas, 5 lanes", 7, differ(b, a[perm]), None, 0)
    assert differ(b, a[perm]) == 0, (a, b)


def test_lane_workspaces_reused_across_shapes(ctx, ctx2):
    """2046 x 8, then 1489 x 4, then 2046 x 8 again on the same lanes: the third call has the first call's bits (and each its single fits')."""
    t = "test_lane_workspaces_reused_across_shapes"
    a, b = th.scan_case("scan-S8"), th.scan_case("scan-S4")
    prime(ctx, ctx2, a, a["thetas"])
    prime(ctx, ctx2, b, b["thetas"])
    first = grid(ctx, a, a["thetas"], 5)
    mid = grid(ctx, b, b["thetas"], 5)
    third = grid(ctx, a, a["thetas"], 5)
    assert_grid_is_single(t, ctx2, b, b["thetas"], mid, 5, "trend_one_launch_per_pass = 1")
    assert_grid_is_single(t, ctx2, a, a["thetas"], third, 5, "trend_one_launch_per_pass = 1")
    log_record(t, "totals of the third call that differ from the first call's", "scan-S8, scan-S4, scan-S8 | 5 lanes", 5, differ(third, first), None, 0)
    assert differ(third, first) == 0, (first, third)


# ---------------------------------------------------------------------------------------------------------------------------
# d. the total and its NaN rule
# ---------------------------------------------------------------------------------------------------------------------------
def check_total(test, name, sc, cols):
    dev = cols["deviance"]
    n = len(dev)
    assert sc["nAllZero"] == 0 and not cols["allZero"].any() and np.isfinite(dev).all(), name
    exact = math.fsum(dev.tolist())
    bound = (n - 1) * 2.0 ** -53 * math.fsum(np.abs(dev).tolist())
    err = abs(sc["sumDeviance"] - exact)
    log_record(test, "sumDeviance against math.fsum of the reported deviance column, absolute", name, n, err, None, bound)
    assert err <= bound, (name, sc["sumDeviance"], exact, err, bound)


@pytest.mark.parametrize("n", th.SUM_SIZES)
def test_total_is_the_sum_of_the_reported_deviances(ctx, n):
    """dev_sum_kernel, one block of 256 threads over the block partials of wald_intercept_kernel, at 1, 255, 256, 257 and 1025 rows (trend
    and prior pinned): within the bound of any summation order of the fit's own reported column — at one row, that row's deviance."""
    from chicdiff_amd import hip
    case = th.sum_case(n)
    S = case["counts"].shape[1]
    dk, dF = ctx.to_device(case["counts"], np.int32), ctx.to_device(case["FullMean"], np.float64)
    out, sc = ctx.nbglm_fit(dk, ctx.offsets(dF, case["sf"], case["theta"]), np.zeros(S, dtype=np.int32), want=["deviance", "allZero"],
                            opts=hip.default_opts(**case["opts"]))
    check_total("test_total_is_the_sum_of_the_reported_deviances", case["name"], sc, {k: v.cpu().numpy() for k, v in out.items()})


def test_total_of_a_free_scan_fit(ctx):
    case = th.scan_case("scan-S8")
    _, sc, cols = single(ctx, case, 0.5, want=("deviance", "allZero"))
    check_total("test_total_of_a_free_scan_fit", "scan-S8, theta = 0.5", sc, cols)


def test_all_zero_rows_make_every_total_na(ctx, tmp_path):
    """sum(mcols$deviance) without na.rm: three all-zero rows (first, middle, last) make every total of the grid NaN, on the parent and on
    the lanes; the single fit says how many there are; DESeq2Wrap of the mirror stops with its message."""
    t = "test_all_zero_rows_make_every_total_na"
    case = th.scan_case("scan-zero")
    dk, dF = on_device(ctx, case)
    for lanes in (1, 5):
        with options(ctx, theta_grid_concurrency=lanes):
            g = ctx.theta_grid(dk, dF, case["sf"], case["thetas"])
        log_record(t, "totals that are not NaN", f"scan-zero | {lanes} lanes", len(g), int(np.sum(~np.isnan(g))), None, 0)
        assert np.isnan(g).all(), (lanes, g)
    total, sc, cols = single(ctx, case, 0.5, want=("deviance", "allZero"))
    assert np.isnan(total) and sc["nAllZero"] == 3 and sc["status"] & 8, sc
    assert np.array_equal(np.flatnonzero(cols["allZero"]), case["planted"]["zero"]) and np.array_equal(np.flatnonzero(np.isnan(cols["deviance"])), case["planted"]["zero"])
    from chicdiff_amd.deseq2wrap import DESeq2Wrap
    RU, long, rmapfile, counts, *_ = tgp._make_tables(600, 8, 3, tmp_path)
    n = len(counts)
    long = long.copy()
    long.loc[long["regionID"].isin([1, n // 2, n]), "N"] = 0
    settings = {"norm": "combined", "theta": None, "theta_grid": [0, 0.25, 0.5, 0.75, 1], "rmapfile": rmapfile, "saveAuxData": False, "outprefix": str(tmp_path / "x")}
    with pytest.raises(ValueError, match="zero counts in every sample"):
        DESeq2Wrap(settings, RU, long, ctx=ctx)
