"""The results stage of the device (cooks_filter_kernel, the if_* kernels with lowess_host, the bh_* kernels, the ihw_* kernels) against
exact rationals and 50-digit arithmetic: the judge of tests/test_results_twin.py on the small cases of tests/results_inputs.py.

tests/test_gpu_parity.py holds these entry points to tests/results_twin.py and to the CPU oracle on continuous random inputs and on one
real table; here the same calls run on inputs with the edges planted (p-values on the BH edge, ties across wave and workgroup edges,
quantile positions inside runs of tied baseMean and on integer h, numRej profiles that steer the threshold rule, log|avDist| within an
ulp of a break), and every element is compared with tests/results_exact_twin.py, which shares no code with either.  The exact
requirements hold on every element; per value stratum the device's worst error must stay within ALLOWANCE x max(the yardstick's worst
on the same elements in the same run, FLOOR) — 4 and 1 unit, the constants of tests/test_gpu_disp.py.  Nothing else is fixed in advance.

Every comparison goes to test_gpu_parity.PARITY_LOG (profiles/r32_results_accuracy.json holds the records of one run), and with it
every decision the device takes another way than exact arithmetic does, with its margin.
"""
import numpy as np
import pytest

import results_inputs as ri
import results_twin as yard
import test_results_twin as tr
from test_gpu_disp import ALLOWANCE, FLOOR
from test_gpu_objective import log_record
from test_norm_twin import Verdict

pytestmark = pytest.mark.gpu


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


class DeviceEngine:
    """the calls of test_results_twin.YardEngine on a HipContext; host arrays in, host arrays out"""

    def __init__(self, ctx):
        self.ctx = ctx

    def dev(self, a, dtype=np.float64):
        return self.ctx.torch.as_tensor(np.ascontiguousarray(a, dtype=dtype)).to(self.ctx.device)

    def filtering(self, bm, p, alpha):
        padj, info = self.ctx.independent_filtering(self.dev(bm), self.dev(p), alpha)
        return padj.cpu().numpy(), info

    def cooks(self, case):
        """as deseq2wrap.py calls it: only where some group has three samples"""
        g = np.asarray(case["group"])
        pv = self.dev(case["pvalue"])
        if len(g) <= 2 or max(int((g == 0).sum()), int((g == 1).sum())) < 3:
            return pv.cpu().numpy(), 0
        nout = self.ctx.cooks_filter(self.ctx.to_device(case["counts"], np.int32), g, self.dev(case["maxCooks"]), self.dev(case["argmax"], np.int32), pv,
                                     case["cutoff"])
        return pv.cpu().numpy(), nout

    def bh(self, p):
        return self.ctx.bh_adjust(self.dev(p)).cpu().numpy()

    def ihw(self, av, pv, breaks, w):
        out = self.ctx.ihw_apply(self.dev(av), self.dev(pv), breaks, w)
        return tuple(out[k].cpu().numpy() for k in ("group", "weight", "weighted_pvalue", "weighted_padj"))


def check(test, case, dev, ora, n=None, strata=True):
    """dev, ora: verdicts of the device and of the yardstick on the same elements.  Exact requirements on every element; the caps on
    excused decisions; per stratum the device within ALLOWANCE x max(yardstick, FLOOR).  Returns the strata that fail."""
    log_record(test, "violations of the exact requirements", case, sum(len(v) for v in dev.errors.values()), len(dev.violations), len(ora.violations), 0)
    assert not dev.violations, (case, dev.violations[:10])
    assert not ora.violations, (case, "the yardstick itself", ora.violations[:10])
    sd, so = dev.stats, ora.stats
    if "index_excused" in sd:
        log_record(test, "a chosen index that differs from the twin's with a decision within 64 units behind it", case, sd["index_decisions"], sd["index_excused"],
                   so["index_excused"], tr.NEAR_CAP * sd["index_decisions"])
        log_record(test, "filters whose cut has a baseMean in its band and whose rows the candidate took the other way than exact arithmetic "
                   f"(filter, distance in units): device {sd['band_taken_other']}, yardstick {so['band_taken_other']}", case, sd["band_filters"],
                   len(sd["band_taken_other"]), len(so["band_taken_other"]), sd["band_filters"])
        log_record(test, "lowess values not judged (1): the robustness weights are read off residuals at rounding level", case, 50, int(sd["lowess_ill"]), int(so["lowess_ill"]), 1)
        log_record(test, "BH decisions on which the IEEE sequence and exact arithmetic part (a statistic of the input)", case, 0, sd["ieee_exact_disagree"], None, 0)
    if "group_excused" in sd:
        log_record(test, f"groups that differ from the twin's within 2 ulp of a break (row, ulps): device {sd['group_excused'][:8]}, yardstick {so['group_excused'][:8]}",
                   case, sd["group_near"], len(sd["group_excused"]), len(so["group_excused"]), tr.NEAR_CAP * n)
    tr.caps_met(case, dev, n)
    return check_strata(test, case, dev, ora) if strata else []


def check_strata(test, case, dev, ora):
    wd, wo = dev.worst(), ora.worst()
    failed = []
    for key, (w, cnt) in sorted(wd.items()):
        assert key in wo and wo[key][1] == cnt, (case, key, "the yardstick was judged on other elements")
        allowed = ALLOWANCE * max(wo[key][0], FLOOR)
        log_record(test, f"{key[0]}, units of tests/results_exact_twin.py", f"{case} | {key[1]}", cnt, w, wo[key][0], allowed)
        if not w <= allowed:
            failed.append((case, key, w, wo[key][0]))
    return failed


_IF = {}


def run_if(ctx, name):
    """(verdict of the device, verdict of the yardstick), once per case and session"""
    if name not in _IF:
        case = ri.if_case(name)
        _IF[name] = (tr.judge_filtering(case, *DeviceEngine(ctx).filtering(case["baseMean"], case["pvalue"], case["alpha"])),
                     tr.judge_filtering(case, *yard.independent_filtering(case["baseMean"], case["pvalue"], case["alpha"])))
    return _IF[name]


@pytest.mark.parametrize("name", ri.IF_CASES)
def test_independent_filtering_against_twin(ctx, name):
    """the exact requirements of one case: the 50 rejection counts, the chosen index, the NA pattern and the bits of padj, exact thetas
    and thresholds; its value errors go on record and are held in test_filtering_value_strata_pooled_over_the_cases"""
    dev, ora = run_if(ctx, name)
    check("test_independent_filtering_against_twin", name, dev, ora, strata=False)
    for key, (w, cnt) in sorted(dev.worst().items()):
        yard_w = ora.worst()[key][0]
        log_record("test_independent_filtering_against_twin", f"{key[0]}, units of tests/results_exact_twin.py (on record; held over all cases)", f"{name} | {key[1]}",
                   cnt, w, yard_w, ALLOWANCE * max(yard_w, FLOOR))


def test_filtering_value_strata_pooled_over_the_cases(ctx):
    """theta, filterThreshold and lowess (by whether the smoother ran its four passes or stopped after the first: a profile with a
    step) over all cases: the device's worst within ALLOWANCE x max(the yardstick's worst on the same elements, FLOOR).  One case
    holds 50 fitted values and one threshold; a stratum pooled over the cases is what the two implementations can be compared on."""
    dev, ora = Verdict(), Verdict()
    for name in ri.IF_CASES:
        d, o = run_if(ctx, name)
        dev.merge(d); ora.merge(o)
    failed = check_strata("test_filtering_value_strata_pooled_over_the_cases", "all cases", dev, ora)
    assert not failed, failed


@pytest.mark.parametrize("name", list(ri.COOKS_DESIGNS))
def test_cooks_filter_against_twin(ctx, oracle, name):
    """which rows lose their p-value, and how many: the cutoff and its two neighbouring doubles, NaN, the rescue at exactly 2 and 3"""
    case = ri.cooks_case(name)
    dev = tr.judge_cooks(case, *DeviceEngine(ctx).cooks(case))
    ora = tr.judge_cooks(case, *tr.YardEngine(oracle).cooks(case))
    log_record("test_cooks_filter_against_twin", "rows whose p-value or NA differs from the twin's, and the count", name, len(case["pvalue"]), len(dev.violations),
               len(ora.violations), 0)
    assert not dev.violations, dev.violations
    assert not ora.violations, ora.violations


@pytest.mark.parametrize("name", ri.IHW_CASES)
def test_ihw_and_bh_against_twin(ctx, oracle, name):
    """group, weight, weighted_pvalue, weighted_padj; and bh_adjust on the case's p-values"""
    case = ri.ihw_case(name)
    eng = DeviceEngine(ctx)
    args = (case["avDist"], case["pvalue"], case["breaks"], case["weights"])
    dev, ora = tr.judge_ihw(case, *eng.ihw(*args)), tr.judge_ihw(case, *oracle.ihw_apply(*args))
    failed = check("test_ihw_and_bh_against_twin", name, dev, ora, len(case["avDist"]))
    assert not failed, failed
    b = Verdict()
    tr.judge_bh(b, "bh_adjust", case["pvalue"], eng.bh(case["pvalue"]))
    log_record("test_ihw_and_bh_against_twin", "bh_adjust: values that are not the bits of the IEEE sequence", name, len(case["pvalue"]), len(b.violations), 0, 0)
    assert not b.violations, b.violations


def test_257_groups_are_refused(ctx):
    eng = DeviceEngine(ctx)
    with pytest.raises(RuntimeError, match="bad arguments"):
        eng.ihw(np.full(4, 10.0), np.full(4, 0.5), np.arange(258, dtype=np.float64), np.ones(257))


def test_nan_basemean_is_refused(ctx):
    """quantile() stops on a missing baseMean in R; so does the entry point"""
    eng = DeviceEngine(ctx)
    bm = np.array([1.0, 2.0, np.nan, 4.0] * 300)
    with pytest.raises(RuntimeError, match="NaN baseMean"):
        eng.filtering(bm, np.linspace(0.001, 1.0, len(bm)), 0.1)
    padj, info = eng.filtering(np.nan_to_num(bm, nan=3.0), np.linspace(0.001, 1.0, len(bm)), 0.1)   # the context is usable afterwards
    assert info["index"] >= 1 and np.isfinite(padj).any()


def test_chain_against_twin(ctx, oracle):
    """the S8-4v4 case of tests/wald_inputs.py fitted on the device with its pinned trend and prior; its own baseMean, pvalue, maxCooks
    and cooksArgmax through Cook's filter, independent filtering and ihw_apply with seven made-up groups, each stage judged on what
    it was really given; the yardstick runs the same chain on the same fit"""
    import wald_inputs as wi
    from test_gpu_wald import device_fit
    case = wi.make_case("S8-4v4")
    fit, _ = device_fit(ctx, case["counts"], case["nf"], case["group"], case["opts"])
    dev = tr.run_chain(DeviceEngine(ctx), fit, case["group"], case["counts"])
    ora = tr.run_chain(tr.YardEngine(oracle), fit, case["group"], case["counts"])
    failed = []
    assert not dev["cooks"].violations and not ora["cooks"].violations, (dev["cooks"].violations, ora["cooks"].violations)
    for stage in ("filtering", "ihw"):
        failed += check("test_chain_against_twin", f"chain {stage}", dev[stage], ora[stage], len(case["counts"]))
    assert not failed, failed
    log_record("test_chain_against_twin", f"rows Cook's filter set to NA, NA padj, chosen index: {dev['facts']}", "chain", len(case["counts"]),
               dev["facts"]["outliers"], ora["facts"]["outliers"], ora["facts"]["outliers"])
    assert dev["facts"] == ora["facts"]
