"""The Wald stage of the device fit (wald_prep_kernel -> wald_irls_kernel -> wald_final_kernel / wald_intercept_kernel) against
50-digit arithmetic: the judge of tests/test_wald_twin.py on the small cases of tests/wald_inputs.py.

tests/test_gpu_parity.py holds these columns to the project's own CPU oracle at 1e-6 (maxCooks 1e-5) and never looks at cooksArgmax or
interceptSE.  Here every row's step count, iterate, standard errors, stat, p, largest Cook's distance and its position are compared
with tests/wald_twin.py, which shares no code with either.  Integer and bit-exact requirements hold on every row; for the rest, per
stratum (quantity, row class), the device's worst error must stay within ALLOWANCE x max(the oracle's worst on the same inputs in the
same run, 1 unit) — 4, as for the dispersion objective (tests/test_gpu_objective.py) and for the same reasons: table-driven 1-ulp
texp / tlog and rcp against libm and IEEE division, sums folded in another order.  Nothing else is fixed in advance.

The dispersion-stage columns that COLUMNS leaves out (baseMean, baseVar, dispGeneEst, dispFit, dispMAP, dispGeneIter, dispIter,
dispOutlier) have a judge of their own: tests/disp_twin.py, tests/test_disp_twin.py and tests/test_gpu_disp.py.

Every comparison goes to test_gpu_parity.PARITY_LOG (profiles/r23_wald_accuracy.json holds the records of one run).
"""
import numpy as np
import pytest

import test_gpu_parity as tgp
import test_wald_twin as tw
import wald_inputs as wi
from test_gpu_objective import log_record

pytestmark = pytest.mark.gpu

ALLOWANCE = 4.0   # x the oracle's worst error in the stratum ...
FLOOR = 1.0       # ... or x one unit, where the oracle does better than that
WANT = tgp.WANT + ["cooksArgmax"]
COLUMNS = [k for k in WANT if k not in ("baseMean", "baseVar", "dispGeneEst", "dispFit", "dispMAP", "dispGeneIter", "dispIter", "dispOutlier")]


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
    from chicdiff_amd import hip
    dk, dn = ctx.to_device(counts, np.int32), ctx.to_device(nf, np.float64)
    out, sc = ctx.nbglm_fit(dk, dn, group, want=WANT, opts=hip.default_opts(**opts))
    return {k: v.cpu().numpy() for k, v in out.items()}, sc


_RUNS = {}


def run_case(ctx, oracle, name):
    """(case, device columns, judge of the device, judge of the oracle), once per case and session."""
    if name not in _RUNS:
        case = wi.make_case(name)
        got, _ = device_fit(ctx, case["counts"], case["nf"], case["group"], case["opts"])
        ref = tw.columns(oracle.nbglm_fit(case["counts"], case["nf"], case["group"], **case["opts"]))
        _RUNS[name] = (case, got, tw.judge(case, got), tw.judge(case, ref))
    return _RUNS[name]


def check_strata(test, dev, ora):
    """dev, ora: {case: judge result}.  Per stratum: the device within ALLOWANCE x max(oracle, FLOOR); the oracle's strata are divided as
    the device's (a small stratum is pooled over the cases given).  Returns the strata that fail."""
    sd, own = tw.pooled(dev)
    so, _ = tw.pooled(ora, own)
    failed = []
    for key, (w, n, at) in sorted(sd.items()):
        yard = so[key][0] if key in so else None
        allowed = ALLOWANCE * max(yard if yard is not None else 0.0, FLOOR)
        log_record(test, f"{key[1]}, units of tests/wald_twin.py", f"{key[0]} | {key[2]}", n, w, yard, allowed)
        if not w <= allowed:
            failed.append((key, w, yard, at))
    return failed


def integer_requirements(name, res, n):
    assert not res["violations"], (name, res["violations"][:10])
    assert res["near"] <= tw.NEAR_CAP * n, (name, res["near"])


@pytest.mark.parametrize("name", list(wi.DESIGNS))
def test_wald_against_twin(ctx, oracle, name):
    """One case of wald_inputs.DESIGNS: the device's Wald columns under the judge, the oracle's as the yardstick.  Strata of fewer than
    20 rows are left to test_wald_small_strata_pooled_over_the_cases."""
    case, got, dev, ora = run_case(ctx, oracle, name)
    n = len(case["counts"])
    log_record("test_wald_against_twin", "rows whose step count differs from the twin's by one, at a conv_test within 1e-3 of betaTol", name, n,
               dev["near"], ora["near"], tw.NEAR_CAP * n)
    log_record("test_wald_against_twin", "violations: step count, stat != lfc / lfcSE bit for bit, arg-max, all-zero rows", name, n,
               len(dev["violations"]), len(ora["violations"]), 0)
    integer_requirements(name, dev, n)
    assert not ora["violations"], (name, "the yardstick itself", ora["violations"][:10])
    big = lambda r: dict(r, errors={k: v for k, v in r["errors"].items() if len(v) >= tw.SMALL_STRATUM})
    big_dev = big(dev)
    failed = check_strata("test_wald_against_twin", {name: big_dev}, {name: dict(ora, errors={k: v for k, v in ora["errors"].items() if k in big_dev["errors"]})})
    assert not failed, failed


def test_wald_small_strata_pooled_over_the_cases(ctx, oracle):
    """The strata too small to stand alone in their case (rows that took 20-99 steps, rows the optimiser finished, ...), pooled by
    (quantity, row class) over all cases: the same bound."""
    runs = {name: run_case(ctx, oracle, name) for name in wi.DESIGNS}
    small = lambda r: dict(r, errors={k: v for k, v in r["errors"].items() if len(v) < tw.SMALL_STRATUM})
    dev = {name: small(r[2]) for name, r in runs.items()}
    ora = {name: dict(r[3], errors={k: v for k, v in r[3]["errors"].items() if k in dev[name]["errors"]}) for name, r in runs.items()}
    failed = check_strata("test_wald_small_strata_pooled_over_the_cases", dev, ora)
    assert not failed, failed


def test_wald_copies_of_a_row_agree(ctx, oracle):
    """Eight hard rows stand four times in every case — where they were planted, and at the first, a middle and the last row positions
    (other lanes, other waves, other blocks, the partial last wave): every output column of a copy has the original's bits."""
    differ = []
    for name in wi.DESIGNS:
        case, got, _, _ = run_case(ctx, oracle, name)
        p = case["planted"]
        for k in WANT:
            for dst in p["copies"]:
                same = tw.same_bits(got[k][dst].astype(np.float64), got[k][p["hard"]].astype(np.float64))
                differ += [(name, k, int(d), int(h)) for d, h, s in zip(dst, p["hard"], same) if not s]
    log_record("test_wald_copies_of_a_row_agree", "output values that differ between copies of a row", "9 cases x 8 rows x 3 copies", 9 * 24 * len(WANT),
               len(differ), None, 0)
    assert not differ, differ[:10]


def test_wald_rows_do_not_depend_on_their_neighbours(ctx, oracle):
    """The 599 rows of the 4 v 4 case 512 times over: 306 688 rows, more than the 196 608 lanes the IRLS launch holds, so rows start from
    the queue's refill as well as from the first fill, and the launch ends in the samples-across-lanes tick with the 20-100 step rows
    that are left.  Every copy of a row must have, in every Wald column, the bits of that row in the first tile; 200 sampled rows pass the
    judge.  (No comparison with the 599-row run: varLogDispEsts, and with it dispOutlier, depends on the row set.)"""
    case = wi.make_case("S8-4v4")
    n0, tiles = len(case["counts"]), 512
    counts, nf = np.tile(case["counts"], (tiles, 1)), np.tile(case["nf"], (tiles, 1))
    got, _ = device_fit(ctx, counts, nf, case["group"], case["opts"])
    differ = {}
    for k in COLUMNS:
        v = got[k].astype(np.float64).reshape(tiles, n0)
        bad = ~tw.same_bits(v, np.broadcast_to(v[0], v.shape))
        if bad.any():
            differ[k] = (int(bad.sum()), [(int(t), int(i)) for t, i in np.argwhere(bad)[:5]])
    log_record("test_wald_rows_do_not_depend_on_their_neighbours", "values that differ from the row's copy in the first tile", f"{tiles} x {n0} rows x {len(COLUMNS)} columns",
               tiles * n0 * len(COLUMNS), sum(c for c, _ in differ.values()), None, 0)
    assert not differ, differ
    rng = np.random.default_rng(2301)
    p = case["planted"]
    base = np.concatenate([p["slow"][:10], p["huge"][:10], p["tie"][:6], p["zero"][:1], rng.choice(n0, 173, replace=False)])
    rows = base + n0 * rng.integers(1, tiles, len(base))
    big = dict(case, counts=counts, nf=nf)
    dev = tw.judge(big, got, rows)
    ref = tw.columns(oracle.nbglm_fit(case["counts"], case["nf"], case["group"], **case["opts"]))
    ora = tw.judge(case, ref, base)
    integer_requirements("S8-4v4 tiled", dev, len(rows))
    failed = check_strata("test_wald_rows_do_not_depend_on_their_neighbours", {"S8-4v4 tiled": dev}, {"S8-4v4 tiled": ora})
    assert not failed, failed
