"""The normalisation stage of the device (fragment_background_kernel, window_sums_kernel, the sf_* kernels on both select routes,
offsets16_kernel<4/8/16>, offsets_kernel for S > 16, and region_assemble_kernel) against 50-digit arithmetic: the judge of
tests/test_norm_twin.py on the small cases of tests/norm_inputs.py.

tests/test_gpu_parity.py and tests/test_size_factors_direct.py hold these steps to the project's own CPU oracle at rtol = 1e-13 on one
benign input each (window sums: 11 fragments per region everywhere; offsets: S = 8 only, the S > 16 kernel against nothing).  Here the
same calls run on inputs with the edges planted, and every element is compared with tests/norm_twin.py, which shares no code with
either: the exact requirements (N sums, NaN / Inf places, which rows take the size factors, Tmean bits) hold on every element; for the
rest, per stratum (quantity, row class), the device's worst error must stay within ALLOWANCE x max(the oracle's worst on the same
elements in the same run, FLOOR) — 4 and 1 unit, the constants of tests/test_gpu_disp.py, for the reasons given there.  Nothing else
is fixed in advance.

Every comparison goes to test_gpu_parity.PARITY_LOG (profiles/r29_norm_accuracy.json holds the records of one run).
"""
import numpy as np
import pytest

import norm_inputs as ni
import norm_twin as nt
import test_norm_twin as tn
from test_gpu_disp import ALLOWANCE, FLOOR
from test_gpu_objective import log_record

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
    """the calls of test_norm_twin.OracleEngine on a HipContext; host arrays in, host arrays out"""

    def __init__(self, ctx):
        self.ctx = ctx

    def dev(self, a, dtype):
        return self.ctx.torch.as_tensor(np.ascontiguousarray(a, dtype=dtype)).to(self.ctx.device)

    def background_tensors(self, args):
        d = self.dev
        return (d(args["bait"], np.int32), d(args["oe"], np.int32), int(args["id_min"]), d(args["midsum"], np.int64), d(args["sj"], np.float64),
                d(args["si"], np.float64), d(args["tblb"], np.int32), d(args["tlb"], np.int32), d(args["T"], np.float64), args["distfun"])

    def background(self, args, only_fullmean=False):
        outs = self.ctx.fragment_background(*self.background_tensors(args), only_fullmean=only_fullmean)
        return [None if t is None else t.cpu().numpy() for t in outs]

    def sums(self, fn, fm, ptr):
        N, FM = self.ctx.window_sums(None if fn is None else self.ctx.to_device(fn, np.int32), None if fm is None else self.ctx.to_device(fm, np.float64),
                                     self.dev(ptr, np.int64))
        return (None if N is None else N.cpu().numpy().T), (None if FM is None else FM.cpu().numpy().T)

    def size_factors(self, counts):
        return self.ctx.size_factors(self.ctx.to_device(counts, np.int32))

    def offsets(self, fm, sf, theta):
        return self.ctx.offsets(self.ctx.to_device(fm, np.float64), sf, theta).cpu().numpy().T


def check_strata(test, case, dev, ora):
    """dev, ora: verdicts of the device and of the oracle on the same elements.  Exact requirements on every element; per stratum the
    device within ALLOWANCE x max(oracle, FLOOR).  Returns the strata that fail."""
    log_record(test, "violations of the exact requirements (patterns, N sums, Tmean bits, copies)", case, sum(len(v) for v in dev.errors.values()),
               len(dev.violations), len(ora.violations), 0)
    assert not dev.violations, (case, dev.violations[:10])
    assert not ora.violations, (case, "the yardstick itself", ora.violations[:10])
    wd, wo = dev.worst(), ora.worst()
    failed = []
    for key, (w, n) in sorted(wd.items()):
        assert key in wo and wo[key][1] == n, (case, key, "the oracle was judged on other elements")
        yard = wo[key][0]
        allowed = ALLOWANCE * max(yard, FLOOR)
        log_record(test, f"{key[0]}, units of tests/norm_twin.py", f"{case} | {key[1]}", n, w, yard, allowed)
        if not w <= allowed:
            failed.append((case, key, w, yard))
    return failed


@pytest.mark.parametrize("S", ni.A3_S)
def test_fragment_background_against_twin(ctx, oracle, S):
    """Bmean, Tmean and FullMean of every planted row and replicate; FullMean alone (only_fullmean=True) has the same bits."""
    case = ni.a3_case(S)
    eng = DeviceEngine(ctx)
    B, Tm, F = eng.background(case["args"])
    dev = tn.judge_a3(S, case, B, Tm, F)
    ora = tn.judge_a3(S, case, *tn.OracleEngine(oracle).background(case["args"]))
    failed = check_strata("test_fragment_background_against_twin", f"S = {S}", dev, ora)
    assert not failed, failed
    b, t, f = eng.background(case["args"], only_fullmean=True)
    assert b is None and t is None and np.all(tn.same_bits(f, F))


@pytest.mark.parametrize("mode", tn.A2_MODES)
@pytest.mark.parametrize("name", ni.A2_CASES)
def test_window_sums_against_twin(ctx, oracle, name, mode):
    """staged blocks, direct-path blocks (more than kWinCap fragments under 256 regions), empty and ragged regions, NaN / Inf fragments"""
    case, dev = tn.run_a2(DeviceEngine(ctx), name, mode)
    _, ora = tn.run_a2(tn.OracleEngine(oracle), name, mode)
    failed = check_strata("test_window_sums_against_twin", f"{name}, {mode}", dev, ora)
    assert not failed, failed


def test_size_factors_against_twin_on_both_routes(ctx, oracle):
    """the direct select (default) and the radix select over stored keys (option select_all_rounds = 1, on a second context)"""
    from chicdiff_amd import hip
    classic = hip.HipContext(0)
    classic.set_option("select_all_rounds", 1)
    try:
        failed = []
        for route, c in (("direct select", ctx), ("radix select", classic)):
            dev, ora = tn.Verdict(), tn.Verdict()
            for name, counts in ni.a5_cases().items():
                dev.merge(tn.judge_a5(name, counts, DeviceEngine(c).size_factors(counts)))
                ora.merge(tn.judge_a5(name, counts, oracle.size_factors(counts)))
            failed += check_strata("test_size_factors_against_twin_on_both_routes", route, dev, ora)
        assert not failed, failed
    finally:
        classic.set_option("select_all_rounds", 0)
        classic.close()


@pytest.mark.parametrize("S,n", ni.A4_SHAPES)
def test_offsets_against_twin(ctx, oracle, S, n):
    """the class kernels at their edges and the generic kernel, unmixed and at every theta; rows that take the size factors"""
    case = ni.a4_case(S, n)
    dev, ora = tn.Verdict(), tn.Verdict()
    eng = DeviceEngine(ctx)
    for theta in ni.THETAS:
        v, na = tn.judge_a4((S, n), case["fm"], case["sf"], theta, eng.offsets(case["fm"], case["sf"], theta))
        dev.merge(v)
        ora.merge(tn.judge_a4((S, n), case["fm"], case["sf"], theta, oracle.offsets(case["fm"], case["sf"], theta))[0])
        assert na == [nt.row_is_na(r) for r in case["fm"]]
    failed = check_strata("test_offsets_against_twin", f"S = {S}, n = {n}", dev, ora)
    assert not failed, failed


def test_chain_and_region_assemble(ctx, oracle):
    """a3 -> a2 -> a5 -> a4 on one region set, each stage judged on what it was really given; the dist = 0 row's FullMean is +Inf, its
    region's sum +Inf, its offsets the size factors.  region_assemble gives the bits of the three calls it replaces."""
    ch = ni.chained_case()
    eng = DeviceEngine(ctx)
    dev, val = tn.run_chain(eng, ch)
    ora, _ = tn.run_chain(tn.OracleEngine(oracle), ch)
    failed = []
    for stage in ("a3", "a2", "a5", "a4"):
        failed += check_strata("test_chain_and_region_assemble", f"chain {stage}", dev[stage], ora[stage])
    assert not failed, failed
    tn.check_chain_facts(ch, val)
    bg = eng.background_tensors(ch["a3"]["args"])
    bait, oe = bg[0], bg[1]
    tables = [(eng.dev(k, np.int64), eng.dev(v, np.int32)) for k, v in ch["tables"]]
    ptr = eng.dev(ch["region_ptr"], np.int64)
    fragN = ctx.count_join_multi(bait, oe, tables)
    assert np.array_equal(fragN.cpu().numpy().T, ch["fragN"])
    _, _, fragFM = ctx.fragment_background(*bg, only_fullmean=True)
    N3, FM3 = ctx.window_sums(fragN, fragFM, ptr)
    N, FM = ctx.region_assemble(bait, oe, ptr, tables, *bg[2:])
    assert np.array_equal(N3.cpu().numpy().T, val["N"]) and np.all(tn.same_bits(FM3.cpu().numpy().T, val["FM"]))   # the three calls ARE what was judged
    differ = int((N.cpu().numpy() != N3.cpu().numpy()).sum() + (~tn.same_bits(FM.cpu().numpy(), FM3.cpu().numpy())).sum())
    log_record("test_chain_and_region_assemble", "values of region_assemble that differ from the three calls", "N and FullMean", 2 * N.numel(), differ, None, 0)
    assert differ == 0


def test_host_distance_function_on_record():
    """chicEstimateDistFunValues (host, numpy) against the exact least-squares fit: its worst error goes into the same record"""
    for nbins in tn.DISTFUN_BINS:
        w = tn.distfun_worst(nbins)
        log_record("test_host_distance_function_on_record", "fitted distance function (host), units of tests/norm_twin.py", f"{nbins} bins", nbins + 4, w, None,
                   tn.distfun_bound(nbins))
        assert w <= tn.distfun_bound(nbins)
