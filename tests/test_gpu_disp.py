"""The dispersion stage of the device fit (prep -> disp_fit_kernel<gene> -> disp_grid_kernel -> trend + MAD -> disp_fit_kernel<MAP>)
against 50-digit arithmetic: the judge of tests/test_disp_twin.py on the small cases of tests/disp_inputs.py.

tests/test_gpu_parity.py holds dispGeneEst, dispMAP and dispersion to the project's own CPU oracle at 1e-6 (rows outside go to a
referee by the same author), prints the step counts without asserting them, asks of floor rows only "both at the floor", of baseVar
1e-11, of the trend, the MAD and the prior variance 1e-5 .. 1e-7, and never sees alpha_init.  Here every row's step counts, both
estimates, baseMean, baseVar, dispFit, the outlier flag and the final value are compared with tests/disp_twin.py, which shares no code
with either: the gene-wise search replayed from the twin's own alpha_init (so a wrong rough or moments estimate, or a wrong xi, shows
as another path), the MAP search from the REPORTED dispGeneEst and dispFit.  Integer and bit-exact requirements hold on every row; for
the rest, per stratum (quantity, row class), the device's worst error must stay within ALLOWANCE x max(the oracle's worst on the same
rows in the same run, 1 unit) — 4 and 1, as for the dispersion objective (tests/test_gpu_objective.py) and the Wald stage, for the
same reasons.  Nothing else is fixed in advance.

Every comparison goes to test_gpu_parity.PARITY_LOG (profiles/r27_disp_accuracy.json holds the records of one run).
"""
import numpy as np
import pytest

import disp_inputs as di
import test_disp_twin as td
import test_gpu_parity as tgp
from test_gpu_objective import log_record

pytestmark = pytest.mark.gpu

ALLOWANCE = 4.0   # x the oracle's worst error in the stratum ...
FLOOR = 1.0       # ... or x one unit, where the oracle does better than that
STAGE_COLUMNS = ["baseMean", "baseVar", "dispGeneEst", "dispFit", "dispMAP", "dispGeneIter", "dispIter", "dispOutlier"]


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


def device_fit(ctx, counts, nf, group, opts):
    """The device's columns, with the fit's scalars beside them (as the oracle returns them)."""
    from chicdiff_amd import hip
    dk, dn = ctx.to_device(counts, np.int32), ctx.to_device(nf, np.float64)
    out, sc = ctx.nbglm_fit(dk, dn, group, want=tgp.WANT, opts=hip.default_opts(**opts) if opts else None)
    got = {k: v.cpu().numpy() for k, v in out.items()}
    got.update({k: sc[k] for k in ("trendCoef", "varLogDispEsts", "dispPriorVar", "trendOuterIter", "status")})
    return got


_RUNS = {}


def run_case(ctx, oracle, name):
    """(case, device columns, judge of the device, judge of the oracle), once per case and session."""
    if name not in _RUNS:
        case = di.make_case(name)
        got = device_fit(ctx, case["counts"], case["nf"], case["group"], case["opts"])
        ref = td.oracle_columns(oracle, case)
        _RUNS[name] = (case, got, td.judge(case, got, oracle=oracle, device=True), td.judge(case, ref, oracle=oracle))
    return _RUNS[name]


def check_strata(test, dev, ora):
    """dev, ora: {case: judge result}.  Per stratum: the device within ALLOWANCE x max(oracle, FLOOR); the oracle's strata are divided as
    the device's (a small stratum is pooled over the cases given).  Returns the strata that fail."""
    sd, own = td.pooled(dev)
    so, _ = td.pooled(ora, own)
    failed = []
    for key, (w, n, at) in sorted(sd.items()):
        yard = so[key][0] if key in so else None
        allowed = ALLOWANCE * max(yard if yard is not None else 0.0, FLOOR)
        log_record(test, f"{key[1]}, units of tests/disp_twin.py", f"{key[0]} | {key[2]}", n, w, yard, allowed)
        if not w <= allowed:
            failed.append((key, w, yard, at))
    return failed


def _without(res, keep):
    return dict(res, errors={k: v for k, v in res["errors"].items() if keep(k, v)})


@pytest.mark.parametrize("name", list(di.DESIGNS))
def test_disp_against_twin(ctx, oracle, name):
    """One case of disp_inputs.DESIGNS: the device's dispersion-stage columns under the judge, the oracle's as the yardstick.  Strata of
    fewer than 20 rows are left to test_disp_small_strata_pooled_over_the_cases."""
    case, got, dev, ora = run_case(ctx, oracle, name)
    n = dev["stats"]["rows"]
    t = "test_disp_against_twin"
    log_record(t, "rows that agree with the replay only with one near decision taken the other way", name, n, dev["near"], ora["near"], td.NEAR_CAP * n)
    log_record(t, "floor rows (estimate < 1e-6) excused by a near decision", name, n, dev["floor_near"], ora["floor_near"], n)
    log_record(t, "searches whose stop test lies below the objective's rounding and that took another path", name, n, dev["below_rounding"],
               ora["below_rounding"], td.BELOW_ROUNDING_CAP)
    log_record(t, "violations: step counts, allZero pattern, outlier rule, bits of dispersion, bounds", name, n, len(dev["violations"]), len(ora["violations"]), 0)
    assert not dev["violations"], (name, dev["violations"][:10])
    assert dev["near"] <= td.NEAR_CAP * n, (name, dev["near"])
    assert dev["below_rounding"] <= td.BELOW_ROUNDING_CAP, (name, dev["below_rounding"])
    assert not ora["violations"], (name, "the yardstick itself", ora["violations"][:10])
    big_dev = _without(dev, lambda k, v: len(v) >= td.SMALL_STRATUM or k[0] == "varLogDispEsts")
    failed = check_strata(t, {name: big_dev}, {name: _without(ora, lambda k, v: k in big_dev["errors"])})
    assert not failed, failed


def test_disp_small_strata_pooled_over_the_cases(ctx, oracle):
    """The strata too small to stand alone in their case (grid rows, 30-99 steps, ceilings, ...), pooled by (quantity, row class) over
    all cases: the same bound."""
    runs = {name: run_case(ctx, oracle, name) for name in di.DESIGNS}
    dev = {name: _without(r[2], lambda k, v: len(v) < td.SMALL_STRATUM and k[0] != "varLogDispEsts") for name, r in runs.items()}
    ora = {name: _without(r[3], lambda k, v, name=name: k in dev[name]["errors"]) for name, r in runs.items()}
    failed = check_strata("test_disp_small_strata_pooled_over_the_cases", dev, ora)
    assert not failed, failed


def test_disp_copies_of_a_row_agree(ctx, oracle):
    """Eight hard rows stand four times in every case — where they were planted, and at the first, a middle and the last row positions
    (other lanes, other waves, other blocks, the partial last wave): all eight dispersion-stage columns of a copy, and the final
    dispersion, have the original's bits."""
    differ = []
    cols = STAGE_COLUMNS + ["dispersion"]
    for name in di.DESIGNS:
        case, got, _, _ = run_case(ctx, oracle, name)
        p = case["planted"]
        for k in cols:
            for dst in p["copies"]:
                same = td.same_bits(got[k][dst].astype(np.float64), got[k][p["hard"]].astype(np.float64))
                differ += [(name, k, int(d), int(h)) for d, h, s in zip(dst, p["hard"], same) if not s]
    log_record("test_disp_copies_of_a_row_agree", "output values that differ between copies of a row", f"{len(di.DESIGNS)} cases x 8 rows x 3 copies",
               len(di.DESIGNS) * 24 * len(cols), len(differ), None, 0)
    assert not differ, differ[:10]


@pytest.mark.parametrize("name", list(di.FREE_FITS))
def test_global_stage_against_twin(ctx, oracle, name):
    """A free fit: trend coefficients, trendOuterIter, dispFit, varLogDispEsts and dispPriorVar (m - p <= 3: matched by simulation) against the twin on the
    device's own baseMean and dispGeneEst.  Yardstick: oracle.parametric_dispersion_fit and the oracle's MAD on the same columns."""
    fit = di.make_free(name)
    got = device_fit(ctx, fit["counts"], fit["nf"], fit["group"], None)
    assert got["status"] & 1 == 0, got["status"]
    dev = td.judge_global(fit, got, got)
    # the yardstick: the oracle's routines on the DEVICE's columns
    nz = got["allZero"] == 0
    use = nz & (got["dispGeneEst"] > 1e-6)
    coefs, it, rc = oracle.parametric_dispersion_fit(got["baseMean"][use], got["dispGeneEst"][use])
    assert rc == 0
    with np.errstate(divide="ignore"):
        fitted = coefs[0] + coefs[1] / got["baseMean"]
    keep = nz & (got["dispGeneEst"] >= 1e-6)
    x = np.ascontiguousarray(np.log(got["dispGeneEst"][keep]) - np.log(fitted[keep]))
    dev_abs = np.ascontiguousarray(np.abs(x - oracle.lib().oracle_median(oracle._pd(x.copy()), len(x))))
    v = (1.4826 * oracle.lib().oracle_median(oracle._pd(dev_abs), len(x))) ** 2
    m = fit["S"] - 2
    yard_sc = dict(trendCoef=coefs, trendOuterIter=it, varLogDispEsts=v,
                   dispPriorVar=max(v - oracle.lib().oracle_trigamma(m / 2.0), 0.25) if m > 3 else oracle.prior_var_mc(x, m))
    ora = td.judge_global(fit, dict(got, dispFit=fitted), yard_sc)
    t = "test_global_stage_against_twin"
    log_record(t, "violations: trendOuterIter", name, 1, len(dev["violations"]), len(ora["violations"]), 0)
    assert not dev["violations"], dev["violations"]
    assert not ora["violations"], ("the yardstick itself", ora["violations"])
    failed = []
    for q, e in sorted(dev["errors"].items()):
        allowed = ALLOWANCE * max(ora["errors"][q], FLOOR)
        log_record(t, f"{q}, units of tests/disp_twin.py", name, 1, e, ora["errors"][q], allowed)
        if not e <= allowed:
            failed.append((q, e, ora["errors"][q]))
    assert "dispPriorVar" in dev["errors"]  # (m - p <= 3 too: the simulated prior, a grid point, held exactly by judge_global)
    assert not failed, failed

