"""The row-sharded fit at uneven, tiny and degenerate shards, on the real kernels.

tests/test_gpu_sharded.py and the two-rank test of tests/test_gpu_parity.py shard matrices whose row count divides by the world, at
S = 8 and 16, with hundreds of thousands of `synth.make` rows per rank: cnt == maxn on every rank of the all-gather, every rank gives
candidates to every median, no shard is shorter than a tile.  Here the ranks are threads of one process (tests/sharded_transport.py:
one context and one stream per rank out of ONE pool of eight contexts, re-armed per case), the matrices have about 4 000 rows, and the
splits, designs and contents are the ones of tests/sharded_inputs.py — whose preconditions tests/test_sharded_inputs.py asserts on
the CPU.  The reference of every case is the SINGLE-RANK run of the same call on the whole matrix, with the trend kernel capped at
256 // world workgroups on both sides (the order of the trend's sums depends on it); the single-rank fit at these S and edge sizes is
pinned to the 50-digit twins by test_gpu_disp.py, test_gpu_wald.py, test_gpu_norm.py and test_gpu_trend.py.  The reference must have
gone through no refit and report neither a failed nor a local trend.

Results are compared bit for bit, NaN places included; output buffers are pre-filled with different values on the two sides, so a row
that nobody writes shows as a difference."""
import numpy as np
import pytest

import norm_twin
import sharded_inputs as si
from sharded_transport import disarm, run_ranks

pytestmark = pytest.mark.gpu

COLUMNS = ["baseMean", "dispGeneEst", "dispFit", "dispMAP", "dispersion", "dispOutlier", "dispIter", "log2FoldChange", "intercept", "lfcSE",
           "stat", "pvalue", "betaIter", "betaConv", "maxCooks", "cooksArgmax", "allZero"]
ST_TREND_FAILED, ST_TREND_LOCAL = 1, 16
THETAS = [0.0, 0.25, 0.5, 0.75, 1.0]
POOL = 8


@pytest.fixture(scope="module")
def pool():
    import __graft_entry__ as g
    g.build()  # no-op when the in-tree library is up to date
    from chicdiff_amd import hip
    ctxs = [hip.HipContext(0, use_torch_stream=False) for _ in range(POOL)]   # own non-blocking stream each
    yield ctxs
    for c in ctxs:
        c.close()


def rel(a, b):
    return np.abs(a - b) / np.maximum(np.abs(b), 1e-300)


def filled(c, n, value):
    """output buffers for COLUMNS, pre-filled: a row no kernel writes keeps `value`"""
    from chicdiff_amd.hip import OUT_DOUBLE
    t = c.torch
    bufs = {k: t.full((n,), value, dtype=t.float64 if k in OUT_DOUBLE else t.int32, device=c.device) for k in COLUMNS}
    t.cuda.synchronize()   # (filled on torch's stream; the fit writes them on the context's own)
    return bufs


def host(out):
    return {k: out[k].cpu().numpy() for k in COLUMNS}


def scalars(sc):
    """the fit's scalars as (doubles, status)"""
    v = list(sc["trendCoef"]) + [sc["varLogDispEsts"], sc["dispPriorVar"]] + list(sc.get("sizeFactors", []))
    return np.array(v, dtype=np.float64), int(sc["status"])


_refs = {}


def reference(pool, case, zero_rows=True):
    """single-rank runs of the case's calls on the whole matrix (pool[0], disarmed), computed once per case and left unchanged"""
    key = (case, zero_rows)
    if key in _refs:
        return _refs[key]
    inp = si.build(case, zero_rows=zero_rows)
    world, n = len(inp["bounds"]), len(inp["counts"])
    c = pool[0]
    disarm(c)
    c.set_option("trend_persistent_blocks", 256 // world)
    try:
        dk, dF = c.to_device(inp["counts"], np.int32), c.to_device(inp["fm"], np.float64)
        ref = dict(world=world, n=n)
        ref["sf"] = c.size_factors(dk)
        assert c.last_refits() == 0
        out, sc = c.wald_test(dk, dF, inp["group"], theta=0.5, want=COLUMNS, outputs=filled(c, n, -777))
        assert c.last_refits() == 0 and not (sc["status"] & (ST_TREND_FAILED | ST_TREND_LOCAL)), (c.last_refits(), sc["status"])
        ref["wald"], ref["wald_sc"] = host(out), sc
        d_nf = c.offsets(dF, ref["sf"], 0.5)
        ref["nf"] = np.ascontiguousarray(d_nf.cpu().numpy().T)
        out, sc = c.nbglm_fit(dk, d_nf, inp["group"], want=COLUMNS, outputs=filled(c, n, -777))
        assert c.last_refits() == 0 and not (sc["status"] & (ST_TREND_FAILED | ST_TREND_LOCAL)), (c.last_refits(), sc["status"])
        ref["fit"], ref["fit_sc"] = host(out), sc
    finally:
        c.set_option("trend_persistent_blocks", 0)
    _refs[key] = ref
    return ref


def sharded(pool, case, ref, calls=("sf", "wald", "fit"), allgather=True, faults=None, option=None, opts=None, zero_rows=True):
    """the case's calls on every rank; returns the ranks' reports.  faults: {rank: fault_inject bits}, option: (name, value, default)"""
    inp = si.build(case, zero_rows=zero_rows)
    world = len(inp["bounds"])

    def one(c, rank):
        lo, hi = inp["bounds"][rank]
        dk, dF = c.to_device(inp["counts"][lo:hi], np.int32), c.to_device(inp["fm"][lo:hi], np.float64)
        rep = dict(rank=rank, rows=hi - lo)
        c.set_option("trend_persistent_blocks", 256 // world)
        if option:
            c.set_option(option[0], option[1])
        try:
            if "sf" in calls:
                rep["sf"], rep["sf_refits"] = c.size_factors(dk), c.last_refits()
            if "wald" in calls:
                if faults and rank in faults:
                    c.set_option("fault_inject", faults[rank])
                c.enable_timing(1)
                out, sc = c.wald_test(dk, dF, inp["group"], theta=0.5, want=COLUMNS, opts=opts, outputs=filled(c, hi - lo, -555))
                rep["wald"], rep["wald_sc"], rep["wald_refits"] = host(out), sc, c.last_refits()
                rep["collectives"] = {k: tuple(v) for k, v in c.collective_stats().items()}
                c.enable_timing(0)
            if "fit" in calls:
                out, sc = c.nbglm_fit(dk, c.to_device(ref["nf"][lo:hi], np.float64), inp["group"], want=COLUMNS, opts=opts,
                                      outputs=filled(c, hi - lo, -555))
                rep["fit"], rep["fit_sc"], rep["fit_refits"] = host(out), sc, c.last_refits()
        finally:
            c.enable_timing(0)
            c.set_option("fault_inject", 0)
            c.set_option("trend_persistent_blocks", 0)
            if option:
                c.set_option(option[0], option[2])
        return rep

    return run_ranks(pool, world, one, allgather=allgather)


def assert_call_identical(reps, ref, call, want_refits=0):
    """columns concatenated == the reference's, bit for bit; scalars identical on every rank and equal to the reference's; refits"""
    assert [r[call + "_refits"] for r in reps] == [want_refits] * len(reps), (call, [r[call + "_refits"] for r in reps])
    rv, rs = scalars(ref[call + "_sc"])
    for r in reps:
        v, s = scalars(r[call + "_sc"])
        assert np.array_equal(v, rv, equal_nan=True) and s == rs, (call, r["rank"], v, rv, s, rs)
    for k in COLUMNS:
        got = np.concatenate([r[call][k] for r in reps])
        assert got.dtype == ref[call][k].dtype and got.shape == ref[call][k].shape
        same = (got == ref[call][k]) | ((got != got) & (ref[call][k] != ref[call][k]))
        assert same.all(), (call, k, f"{int((~same).sum())} rows differ, first at {int(np.flatnonzero(~same)[0])}",
                            got[~same][:4], ref[call][k][~same][:4])


def assert_collectives(reps, gathers=1):
    """what tests/test_gpu_sharded.py::_check_reports asserts of a plain fit: ONE all-gather, of the rank's padded (x | y) block, and at
    most 8 all-reduces (gathers = 0: no all-gather hook, the trend's rows travel by a sum-all-reduce)"""
    blk = -(-(2 * max(r["rows"] for r in reps) * 8) // 256) * 256
    for r in reps:
        cst = r["collectives"]
        if gathers:
            assert cst["allgather"][0] == 1 and cst["allgather"][2] == blk, (r["rank"], cst, blk)
        else:
            assert cst.get("allgather", (0,))[0] == 0, (r["rank"], cst)
        assert cst["allreduce"][0] <= 8, (r["rank"], cst)


@pytest.mark.parametrize("case", si.CASES, ids=si.case_id)
def test_sharded_calls_equal_the_single_rank_calls(pool, case):
    """Both hooks registered.  `trend_compact_kernel`: cnt[r] < maxn on all ranks but one, blocks gl.block doubles apart (w7: six of
    seven ranks send one row of 4 200); `sel_gcount_kernel` / `sel_gplace_kernel` / `sel_gfinish_kernel` with `sel_gather_layout`: a rank
    without a candidate (zero_shard, no_ratio_shard, the one-row ranks) and a tie run on every rank (ties); `xim_kernel`: the ranks'
    double-double slots in rank order at worlds 3, 5, 7, S = 3 .. 17 and a one-row rank; `prior_mc` with `mad_local` at S = 3, 4, 5 and
    design ~1; the fit kernels on shards of 1, 63, 64, 65, 129, 255, 256, 257, 512, 513, 2048 and 2049 rows, all-zero shards and shards
    with no row usable for the trend (flat_shard)."""
    ref = reference(pool, case)
    reps = sharded(pool, case, ref)
    inp = si.build(case)
    # size_factors, the stand-alone entry point: equal everywhere, the reference's bits, the 50-digit twin within its own bound
    for r in reps:
        assert r["sf_refits"] == 0 and np.array_equal(r["sf"], ref["sf"]), (r["rank"], r["sf"], ref["sf"])
    sf, unit, used = norm_twin.size_factors(inp["counts"])
    err = [abs(float(ref["sf"][j]) - sf[j]) / unit[j] for j in range(inp["S"])]
    print(f"{si.case_id(case)}: size factors vs twin, worst {float(max(err)):.2f} units (bound {norm_twin.bound_sf(inp['S'])}), {used} rows used")
    assert max(err) <= norm_twin.bound_sf(inp["S"]), err
    assert_call_identical(reps, ref, "wald")
    assert_call_identical(reps, ref, "fit")
    assert_collectives(reps)


@pytest.mark.parametrize("case", si.UNEQUAL, ids=si.case_id)
def test_without_the_allgather_hook(pool, case):
    """`gathered_trend`'s sum-all-reduce way (fit_api.hip: `xg + off, yg + off`, off = the lower ranks' counts, over zero-filled
    all-ranks arrays) with unequal counts: the same bits, and no all-gather recorded."""
    ref = reference(pool, case)
    reps = sharded(pool, case, ref, calls=("wald", "fit"), allgather=False)
    assert_call_identical(reps, ref, "wald")
    assert_call_identical(reps, ref, "fit")
    assert_collectives(reps, gathers=0)


@pytest.mark.parametrize("case", si.UNEQUAL, ids=si.case_id)
def test_forced_refits_on_two_ranks(pool, case):
    """`fault_inject` = 4 (size-factor select overflow) on one rank and 1 (fit select overflow) on the last: the verdicts travel with
    the fit's last all-reduce, every rank repeats size factors + fit ONCE, with every histogram round (`sel_hist` / `sel_step` rounds
    over ranks without keys instead of the candidate gather) — the same bits."""
    ref = reference(pool, case)
    world = ref["world"]
    reps = sharded(pool, case, ref, calls=("wald",), faults={(1 if world > 2 else 0): 4, world - 1: 1})
    assert_call_identical(reps, ref, "wald", want_refits=1)


@pytest.mark.parametrize("case", si.UNEQUAL[:2] + [("w7", "S17", "ties", None)], ids=si.case_id)
def test_trend_by_one_allreduce_per_pass(pool, case):
    """`sharded_trend_gather` = 0: `drive_trend` over per-rank partial sums (trend_pass on ranks with one row) and the MAD by the
    sharded selects (`sel_g*` on residual keys, ranks with one or no usable row; ties: both medians of the MAD inside a run of equal
    keys with members on all seven ranks).  The same sums in another order: what
    test_two_ranks_sharing_one_gpu_match_single_rank asserts of it — trendCoef to rtol 1e-10, the same trendOuterIter — and the same
    NaN places; identical on every rank."""
    ref = reference(pool, case)
    reps = sharded(pool, case, ref, calls=("wald",), option=("sharded_trend_gather", 0, 1))
    sc0 = ref["wald_sc"]
    for r in reps:
        sc = r["wald_sc"]
        print(f"{si.case_id(case)} rank {r['rank']}: trendCoef {sc['trendCoef']} vs {sc0['trendCoef']}, refits {r['wald_refits']}")
        assert np.allclose(sc["trendCoef"], sc0["trendCoef"], rtol=1e-10, atol=0) and sc["trendOuterIter"] == sc0["trendOuterIter"]
        assert np.array_equal(sc["trendCoef"], reps[0]["wald_sc"]["trendCoef"])
    for k in COLUMNS:
        got = np.concatenate([r["wald"][k] for r in reps]).astype(np.float64)
        assert np.array_equal(np.isnan(got), np.isnan(ref["wald"][k].astype(np.float64))), k


@pytest.mark.parametrize("case", si.UNEQUAL[:2], ids=si.case_id)
def test_local_trend(pool, case):
    """fitType = 2 (`local_trend_fit`: weighted sums all-reduced per rank, i.e. added in another order than on one rank) on ranks with
    one row: the comparison and the bound of test_two_ranks_sharing_one_gpu_match_single_rank for its `out3`."""
    from chicdiff_amd import hip
    inp = si.build(case)
    ref = reference(pool, case)
    c = pool[0]
    c.set_option("trend_persistent_blocks", 256 // ref["world"])
    try:
        loc, scl = c.wald_test(c.to_device(inp["counts"], np.int32), c.to_device(inp["fm"], np.float64), inp["group"], theta=0.5,
                               opts=hip.default_opts(fitType=2), want=["dispersion"])
    finally:
        c.set_option("trend_persistent_blocks", 0)
    loc = loc["dispersion"].cpu().numpy()
    reps = sharded(pool, case, ref, calls=("wald",), opts=hip.default_opts(fitType=2))
    got = np.concatenate([r["wald"]["dispersion"] for r in reps])
    okl = ~np.isnan(loc)
    assert (scl["status"] & ST_TREND_LOCAL) and all(r["wald_sc"]["status"] == scl["status"] for r in reps)
    assert np.array_equal(np.isnan(got), ~okl)
    rl = rel(got[okl], loc[okl])
    print(f"{si.case_id(case)}: local trend, sharded vs single-rank dispersion: max rel {rl.max():.3e}, share within 1e-9 {np.mean(rl < 1e-9):.5f}")
    assert np.mean(rl < 1e-9) > 0.999 and rl.max() < 1e-4


@pytest.mark.parametrize("case", si.GRID_CASES, ids=si.case_id)
def test_theta_grid_on_sharded_contexts(pool, case):
    """The grid's design-~1 fits, each sharded, one after the other (`chicdiff_hip_theta_grid_dev`, lanes = 1): S = 4 (`prior_mc` with
    `mad_local`, three residual degrees of freedom) on w7 and S = 8 on w4, no all-zero row.  The reference is the single-rank grid called
    with one point at a time (the single-launch trend kernel, as on the ranks).  Each total is a sum of n non-negative per-row
    deviances — the same n numbers when the fits are bit-identical — taken in another order: either order is within (n - 1) 2^-53 of
    the exact sum, relative, so the two differ by at most 2 (n - 1) 2^-53.  The arg-min is the same."""
    inp = si.build(case, zero_rows=False)
    world, n = len(inp["bounds"]), len(inp["counts"])
    c = pool[0]
    disarm(c)
    c.set_option("trend_persistent_blocks", 256 // world)
    try:
        dk, dF = c.to_device(inp["counts"], np.int32), c.to_device(inp["fm"], np.float64)
        sf0 = c.size_factors(dk)
        dev0 = np.array([c.theta_grid(dk, dF, sf0, [t])[0] for t in THETAS])
        assert c.last_refits() == 0
    finally:
        c.set_option("trend_persistent_blocks", 0)
    assert np.all(np.isfinite(dev0)) and np.all(dev0 > 0)

    def one(c, rank):
        lo, hi = inp["bounds"][rank]
        dk, dF = c.to_device(inp["counts"][lo:hi], np.int32), c.to_device(inp["fm"][lo:hi], np.float64)
        c.set_option("trend_persistent_blocks", 256 // world)
        try:
            sf = c.size_factors(dk)
            return sf, c.theta_grid(dk, dF, sf, THETAS), c.last_refits()
        finally:
            c.set_option("trend_persistent_blocks", 0)

    reps = run_ranks(pool, world, one)
    bound = 2 * (n - 1) * 2.0 ** -53
    for rank, (sf, dev, refits) in enumerate(reps):
        worst = float(rel(dev, dev0).max())
        print(f"{si.case_id(case)} rank {rank}: totals {dev.tolist()}, worst rel. difference {worst:.3e} (bound {bound:.3e})")
        assert np.array_equal(sf, sf0) and refits == 0
        assert np.array_equal(dev, reps[0][1])          # all-reduced: the same total on every rank
        assert worst <= bound
        assert int(np.argmin(dev)) == int(np.argmin(dev0))
