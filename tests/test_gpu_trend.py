"""The trend's other branches and the simulated prior on the device against 50-digit arithmetic: the judge of tests/test_trend_twin.py
on the outputs of chicdiff_hip_selftest_global_stage_dev and chicdiff_hip_selftest_resid_hist_dev for every case of tests/trend_inputs.py,
and on three free fits through the product path (judged on the device's own reported baseMean, dispGeneEst and allZero, so that a
mistake in how the fit calls its global stage shows even where the test entry is right).

tests/test_gpu_parity.py compares the local trend, the mean trend and the simulated prior with the project's own CPU oracle — written
by the same hand from the same reading — at rtol 1e-9 .. 3e-4 on one or two benign matrices.  Here: status bits, NaN patterns, vertex
count and order, histogram counts and the prior's argmin exactly; vertex h / f / d, dispFit by class (interior, left- and
right-extrapolated, on a vertex), the mean trend's value, residuals, varLogDispEsts and the closed-form prior per stratum within
ALLOWANCE x max(the oracle's routines on the same columns, FLOOR) — 4 and 1 unit, the constants of tests/test_gpu_disp.py — in the
units of tests/trend_twin.py; excused decisions within the cap of the judge.  Every comparison goes to test_gpu_parity.PARITY_LOG
(profiles/r33_trend_accuracy.json holds the records of one run).
"""
import numpy as np
import pytest

import test_trend_twin as tj
import trend_inputs as ti
import trend_twin as tt
from test_gpu_disp import ALLOWANCE, FLOOR
from test_gpu_objective import log_record

pytestmark = pytest.mark.gpu

_STAGE = dict(tj._CASES)
_WRAP = "grid-wrap-local-S4p2"


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


def device_outputs(ctx, case):
    """The outputs of the global-stage entry on the case's columns, with the histogram kernel's counts of the reported residuals."""
    from chicdiff_amd import hip
    t = ctx.torch
    opts = hip.default_opts(**case["opts"])
    d = [ctx.to_device(np.ascontiguousarray(case[k]), dt) for k, dt in (("baseMean", np.float64), ("dispGeneEst", np.float64), ("allZero", np.int32))]
    ctx.set_option("local_trend_substitute", int(case["substitute"]))
    try:
        r = ctx.selftest_global_stage(d[0], d[1], d[2], case["S"], case["p"], opts)
    except hip.ChicdiffHipError as e:
        assert "no gene-wise estimate above" in str(e), e  # the one error a stage case may end in
        return dict(error=True)
    finally:
        ctx.set_option("local_trend_substitute", 1)
    sc = r["scalars"]
    out = dict(error=False, status=sc["status"], trendCoef=sc["trendCoef"], dispFit=r["dispFit"].cpu().numpy(), resid=r["resid"].cpu().numpy(),
               hist=r["hist"], vertices=r["vertices"], varLogDispEsts=sc["varLogDispEsts"], dispPriorVar=sc["dispPriorVar"])
    out["hist_of_resid"] = ctx.selftest_resid_hist(r["resid"])
    assert t.is_tensor(r["resid"]) and out["resid"].shape == (len(case["baseMean"]),)
    return out


def check(test, name, dev, ora):
    """Exact requirements with no violation, excuses within the cap (inside the judge), every stratum of the device within ALLOWANCE x
    max(yardstick, FLOOR).  Logs every figure."""
    for kind in sorted(set(dev["decisions"]) | set(ora["decisions"])):
        log_record(test, f"decisions of kind '{kind}' excused (near: device {dev['near'].get(kind, 0)})", name, dev["decisions"].get(kind, 0),
                   dev["excused"].get(kind, 0), ora["excused"].get(kind, 0), tj.EXCUSE_CAP * dev["decisions"].get(kind, 0))
    log_record(test, "violations: status bits, NaN patterns, vertices, histogram counts, argmin, trendCoef", name, 1, len(dev["violations"]),
               len(ora["violations"]), 0)
    assert not dev["violations"], (name, dev["violations"][:5])
    assert not ora["violations"], (name, "the yardstick itself", ora["violations"][:5])
    wd, wo = tj.worst(dev), tj.worst(ora)
    failed = []
    for key, (e, row) in sorted(wd.items()):
        yard = wo[key][0] if key in wo else 0.0
        allowed = ALLOWANCE * max(yard, FLOOR)
        log_record(test, f"{key[0]}, units of tests/trend_twin.py", f"{name} | {key[1]}", len(dev["errors"][key]), e, yard, allowed)
        if not e <= allowed:
            failed.append((key, e, yard, row))
    assert not failed, (name, failed)


@pytest.mark.parametrize("name", list(_STAGE) + [_WRAP])
def test_global_stage_entry_against_twin(ctx, oracle, name):
    """One case of tests/trend_inputs.py through chicdiff_hip_selftest_global_stage_dev; the oracle's routines on the same columns are
    the yardstick."""
    case = _STAGE[name] if name in _STAGE else ti.grid_wrap()
    dev = tj.judge(case, device_outputs(ctx, case))
    ora = tj.judge(case, tj.oracle_outputs(oracle, case))
    check("test_global_stage_entry_against_twin", name, dev, ora)


@pytest.mark.parametrize("n", [len(ti.hist_edge_values())] + list(ti.HIST_SIZES))
def test_resid_hist_kernel_counts(ctx, n):
    """chicdiff_hip_selftest_resid_hist_dev on the edge values alone and on columns of 65 535, 65 536, 65 537 and 2 x 65 536 + 1 rows
    (its grid of 256 x 256 threads wraps there) that begin and end with them: the twin's counts on the same doubles, exactly."""
    x = ti.hist_edge_values() if n == len(ti.hist_edge_values()) else ti.hist_column(n)
    got = ctx.selftest_resid_hist(ctx.to_device(x, np.float64))
    bad = tj.judge_hist(x, got)
    log_record("test_resid_hist_kernel_counts", "bins whose count differs from the twin's", f"n = {n}", 40, len(bad), None, 0)
    assert not bad, bad


def _fit_columns(ctx, fit):
    from chicdiff_amd import hip
    dk, dn = ctx.to_device(fit["counts"], np.int32), ctx.to_device(fit["nf"], np.float64)
    want = ["baseMean", "dispGeneEst", "dispFit", "allZero"]
    out, sc = ctx.nbglm_fit(dk, dn, fit["group"], want=want, opts=hip.default_opts(**fit["opts"]) if fit["opts"] else None)
    return {k: v.cpu().numpy() for k, v in out.items()}, sc


@pytest.mark.parametrize("name", ["S8-local", "extreme-substituted"])
def test_free_fit_local_trend_against_twin(ctx, oracle, name):
    """A free fit whose trend is local — on request (S = 8, fitType = 2) and as the substitute for the parametric trend that fails on
    test_gpu_parity._extreme_matrix() — judged on the device's own reported columns: status bits, trendCoef, dispFit by class,
    varLogDispEsts, the closed-form prior."""
    fit = ti.free_fits()[name]
    got, sc = _fit_columns(ctx, fit)
    S = fit["counts"].shape[1]
    case = ti._case(f"free-{name}", got["baseMean"], got["dispGeneEst"], S, 2, fit["opts"], zero=np.flatnonzero(got["allZero"] != 0))
    out = dict(error=False, status=sc["status"], trendCoef=sc["trendCoef"], dispFit=got["dispFit"], varLogDispEsts=sc["varLogDispEsts"],
               dispPriorVar=sc["dispPriorVar"])
    dev = tj.judge(case, out)
    yard = tj.oracle_outputs(oracle, case)
    ora = tj.judge(case, {k: v for k, v in yard.items() if k in out})
    assert tj.expected(case)["status"] & tj.ST_LOCAL
    check("test_free_fit_local_trend_against_twin", name, dev, ora)


def test_free_fit_2v2_simulated_prior_against_twin(ctx, oracle):
    """The reference's own design, S = 4 (2 v 2), through the product path: the parametric trend, varLogDispEsts and the prior variance
    matched by simulation against tests/disp_twin.global_stage on the device's own baseMean and dispGeneEst."""
    import test_disp_twin as td
    fit = ti.free_fits()["S4-2v2"]
    got, sc = _fit_columns(ctx, fit)
    assert sc["status"] & tj.ST_MC and not sc["status"] & (tj.ST_FAILED | tj.ST_LOCAL), sc["status"]
    f = dict(S=4, group=np.asarray(fit["group"]))
    dev = td.judge_global(f, got, sc)
    nz = got["allZero"] == 0
    use = nz & (got["dispGeneEst"] > 1e-6)
    coefs, it, rc = oracle.parametric_dispersion_fit(got["baseMean"][use], got["dispGeneEst"][use])
    assert rc == 0
    with np.errstate(divide="ignore", invalid="ignore"):
        fitted = coefs[0] + coefs[1] / got["baseMean"]
    keep = nz & (got["dispGeneEst"] >= 1e-6)
    x = np.ascontiguousarray(np.log(got["dispGeneEst"][keep]) - np.log(fitted[keep]))
    dev_abs = np.ascontiguousarray(np.abs(x - oracle.lib().oracle_median(oracle._pd(x.copy()), len(x))))
    v = (1.4826 * oracle.lib().oracle_median(oracle._pd(dev_abs), len(x))) ** 2
    yard_sc = dict(trendCoef=coefs, trendOuterIter=it, varLogDispEsts=v, dispPriorVar=oracle.prior_var_mc(x, 2))
    ora = td.judge_global(f, dict(got, dispFit=fitted), yard_sc)
    t = "test_free_fit_2v2_simulated_prior_against_twin"
    log_record(t, "violations: trendOuterIter, argmin of the prior", "S4-2v2", 1, len(dev["violations"]), len(ora["violations"]), 0)
    log_record(t, "argmin of the prior excused by its gap", "S4-2v2", 1, dev["near"], ora["near"], 0)
    assert not dev["violations"] and not ora["violations"], (dev["violations"], ora["violations"])
    assert "dispPriorVar" in dev["errors"]
    failed = []
    for q, e in sorted(dev["errors"].items()):
        allowed = ALLOWANCE * max(ora["errors"][q], FLOOR)
        log_record(t, f"{q}, units of tests/disp_twin.py", "S4-2v2", 1, e, ora["errors"][q], allowed)
        if not e <= allowed:
            failed.append((q, e, ora["errors"][q]))
    assert not failed, failed
