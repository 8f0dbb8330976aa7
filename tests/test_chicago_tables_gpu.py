"""The Chicago background tables on the device against the host twin (pipeline.background_tables, chicdiff.R:656-692, 538-548):
equal in every cell — sj, si and T through their int64 views with NaN in the same cells, tblb and tlb as integers, distfun bit for
bit.  The tables come from tests/chicago_tables_inputs.py (values drawn per row, so the winner of every group shows).
Row orders: WITHOUT repeated (baitID, otherEndID) pairs the keyed, the reversed and the shuffled table hold the same groups with the
same winners, so the three device results must also agree with one another; WITH repeated pairs the winner of a pair is its first
repeat in row order — a property of the table as given — and each table is compared with the twin of that same table."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import chicago_tables_inputs as cti  # noqa: E402

gpu = pytest.mark.gpu
ROWS_PER_WORKGROUP = 4096   # hip.chicago_tables_caps()["rows_per_workgroup"], asserted below: the shapes around it are parametrised


@pytest.fixture(scope="module")
def ctx():
    import __graft_entry__ as g
    g.build()
    from chicdiff_amd import hip
    c = hip.HipContext(0)
    assert hip.chicago_tables_caps()["rows_per_workgroup"] == ROWS_PER_WORKGROUP
    yield c
    c.close()


def host(d):
    return {k: (v.cpu().numpy() if hasattr(v, "cpu") else v) for k, v in d.items()}


def assert_equal_tables(got, want, tag):
    assert got["levB"] == want["levB"] and got["levL"] == want["levL"], tag
    for k in ("sj", "si", "T", "distfun"):
        assert got[k].dtype == np.float64 and cti.same_bits(got[k], want[k]), (tag, k)
    for k in ("tblb", "tlb"):
        assert got[k].dtype == np.int32 and np.array_equal(got[k], want[k]), (tag, k)


def device_and_twin(ctx, xs, nid, tag):
    from chicdiff_amd import pipeline
    want = pipeline.background_tables(xs, cti.ID_MIN, nid)
    got = pipeline.background_tables_dev(xs, cti.ID_MIN, nid, ctx)
    S = len(xs)
    assert got["sj"].shape == (S, nid) and got["tblb"].shape == (S, nid) and got["T"].shape == want["T"].shape and got["sj"].is_cuda
    got = host(got)
    assert_equal_tables(got, want, tag)
    return got, want


@gpu
@pytest.mark.parametrize("n", [1, 64, 65, ROWS_PER_WORKGROUP - 1, ROWS_PER_WORKGROUP + 1, 20011])
def test_equal_to_the_twin_in_every_row_order(ctx, n):
    """n = 1, one wave, one row more, one row fewer and one more than a workgroup takes per pass (4 097 rows), several workgroups."""
    nid = cti.nid_of(n)
    res = [device_and_twin(ctx, [cti.table(n, 1, False, order)], nid, (n, order))[0] for order in cti.ORDERS]
    for order, r in zip(cti.ORDERS[1:], res[1:]):
        assert_equal_tables(r, res[0], (n, order, "against keyed"))
    if n > 1:
        seen = ~np.isnan(res[0]["sj"]) | (res[0]["tblb"] >= 0)
        assert seen.any() and (res[0]["tblb"] == -1).any() and np.isnan(res[0]["T"]).sum() < res[0]["T"].size
    for order in cti.ORDERS:                                            # repeated pairs: the first repeat wins, in each order as given
        device_and_twin(ctx, [cti.table(n, 2, True, order)], nid, (n, order, "repeated pairs"))


@gpu
def test_three_replicates_of_different_length(ctx):
    xs = [cti.table(4097, 1, True), cti.table(65, 2, True, "keyed"), cti.table(20011, 3, False, "reversed")]
    xs[1] = xs[1][xs[1]["tblb"] != cti.LEVB[0]].reset_index(drop=True)   # a replicate that lacks a level the others show
    got, _ = device_and_twin(ctx, xs, 3000, "S = 3")
    assert got["levB"] == sorted(cti.LEVB) and not (got["tblb"][1] == got["levB"].index(cti.LEVB[0])).any()


@gpu
def test_every_slot_contended(ctx):
    """20 000 rows of one bait, 50 other ends and one (tblb, tlb) pair, across workgroups; with the wave-level run merge and without."""
    x = cti.contention()
    try:
        for merge in (1, 0):
            ctx.set_option("chicago_tables_run_merge", merge)
            for order in cti.ORDERS:
                got, _ = device_and_twin(ctx, [cti.reorder(x, order)], 400, ("contention", merge, order))
            assert ((got["tblb"] >= 0) | ~np.isnan(got["sj"])).sum() <= 1 and 25 < ((got["tlb"] >= 0) | ~np.isnan(got["si"])).sum() <= 50
            assert (~np.isnan(got["T"])).sum() <= 1
    finally:
        ctx.set_option("chicago_tables_run_merge", 1)


@gpu
@pytest.mark.parametrize("scattered", [False, True], ids=["consecutive", "scattered"])
def test_tied_pairs_keep_the_first_row(ctx, scattered):
    x, first = cti.ties(scattered)
    got, want = device_and_twin(ctx, [x], 3200, "ties")
    b, o = cti.TIE_BAIT - cti.ID_MIN, cti.TIE_OE - cti.ID_MIN
    assert x["baitID"][first] == cti.TIE_BAIT and (x["baitID"][:first] != cti.TIE_BAIT).all()
    for g in (got, want):                                               # (the generator's promise, on both sides)
        assert g["sj"][0, b] == x["s_j"][first] and g["si"][0, o] == x["s_i"][first]
        assert g["tblb"][0, b] == g["levB"].index(x["tblb"][first]) and g["tlb"][0, o] == g["levL"].index(x["tlb"][first])
    last = int(np.flatnonzero((x["baitID"] == cti.TIE_BAIT).to_numpy())[-1])
    assert x["s_j"][last] != x["s_j"][first]


@gpu
def test_na_at_the_winner_stays_na(ctx):
    x = cti.na_winner()
    got, want = device_and_twin(ctx, [x], 3200, "NA at the winner")
    b = cti.NA_BAIT - cti.ID_MIN
    rows = x[x["baitID"] == cti.NA_BAIT]
    assert rows["s_j"].notna().sum() == 5 and rows["tblb"].notna().sum() == 5
    pair = x[(x["tblb"] == cti.LEVB[0]) & (x["tlb"] == cti.LEVL[0])]
    assert pair["Tmean"].notna().sum() > 10
    for g in (got, want):
        assert np.isnan(g["sj"][0, b]) and g["tblb"][0, b] == -1
        assert not np.isnan(g["si"][0, b + 1])                          # the same row's other columns are values
        assert np.isnan(g["T"][0, g["levB"].index(cti.LEVB[0]), g["levL"].index(cti.LEVL[0])])


@gpu
def test_two_values_under_one_distbin_raise_the_flag(ctx, monkeypatch):
    """The flagged replicate's distance function comes from the host (chicEstimateDistFun, called for it alone); nothing else changes."""
    from chicdiff_amd import pipeline
    xs = [cti.table(4097, 1), cti.not_a_function(), cti.table(65, 2)]
    want = pipeline.background_tables(xs, cti.ID_MIN, 3000)
    calls = []
    real = pipeline.chicEstimateDistFun
    monkeypatch.setattr(pipeline, "chicEstimateDistFun", lambda x, *a, **k: (calls.append(len(x)), real(x, *a, **k))[1])
    got = host(pipeline.background_tables_dev(xs, cti.ID_MIN, 3000, ctx))
    assert calls == [len(xs[1])]
    assert_equal_tables(got, want, "flag")
    clean = host(pipeline.background_tables_dev([cti.table(4097, 6)], cti.ID_MIN, 3000, ctx))
    assert len(calls) == 1
    for k in ("sj", "si", "T"):
        assert cti.same_bits(got[k][1], clean[k][0]), k                 # the changed refBinMean touched the distance function only
    assert not cti.same_bits(got["distfun"][1], clean["distfun"][0])


@gpu
def test_refusals_name_the_limit(ctx):
    from chicdiff_amd import hip
    torch = ctx.torch
    caps = hip.chicago_tables_caps()
    i = lambda n: torch.zeros(n, dtype=torch.int32, device=ctx.device)
    f = lambda *s: torch.zeros(s, dtype=torch.float64, device=ctx.device)
    call = lambda T, ndb, n=8: ctx.chicago_tables(i(n), i(n), f(n), f(n), f(n), f(n), i(n), i(n), i(n), 0, ndb, f(16), f(16), i(16), i(16), T)
    with pytest.raises(ValueError, match=str(caps["max_pairs"])):
        call(f(caps["max_pairs"] // 2 + 1, 2), 4)
    with pytest.raises(ValueError, match=str(caps["max_distbin"])):
        call(f(2, 2), caps["max_distbin"] + 1)
    with pytest.raises(ValueError, match="nrows"):
        call(f(2, 2), 4, n=0)
    with pytest.raises(hip.ChicdiffHipError, match="outside"):          # a tblb code beyond its levels: refused by the library
        ctx.chicago_tables(i(8), i(8), f(8), f(8), f(8), f(8), i(8) + 2, i(8), i(8) - 1, 0, 0, f(16), f(16), i(16), i(16), f(2, 2))
    status = C.c_int32(0)                                               # 2^32 rows: refused on the arguments, no row is read
    rc = ctx.lib.chicdiff_hip_chicago_tables_dev(ctx.h, *([i(8).data_ptr()] * 9), 1 << 32, 0, 16, 2, 2, 4, *([f(16).data_ptr()] * 6), C.byref(status))
    assert rc != 0 and b"2^32" in ctx.lib.chicdiff_hip_last_error(ctx.h)
    ref, flag = call(f(2, 2), 4)                                        # ... and a good call goes through
    assert not flag and ref.shape == (5,)


@pytest.fixture(scope="module")
def experiments(tmp_path_factory):
    from pipeline_inputs import make_experiment
    return {w: make_experiment(tmp_path_factory.mktemp("chin" if w else "nochin"), npeaks=1200, with_chinput=w)[0] for w in (True, False)}


@gpu
@pytest.mark.parametrize("with_chinput,assemble", [(True, False), (True, True), (False, False)],
                         ids=["chinput", "chinput-assemble", "no-chinput"])
def test_mirror_device_tables_same_blocks(ctx, experiments, with_chinput, assemble):
    """getFullRegionData(device_tables=True): every tensor of both blocks equals the device_tables=False run bit for bit."""
    import torch
    from chicdiff_amd import pipeline
    from pipeline_inputs import read_chicago_pickle
    settings = experiments[with_chinput]
    RU = pipeline.getRegionUniverse(settings, ctx)
    RUc = pipeline.getControlRegionUniverse(settings, RU, ctx, rng=np.random.default_rng(11))
    a = pipeline.getFullRegionData(settings, RU, RUc, ctx=ctx, read_chicago=read_chicago_pickle, assemble=assemble)
    b = pipeline.getFullRegionData(settings, RU, RUc, ctx=ctx, read_chicago=read_chicago_pickle, assemble=assemble, device_tables=True)
    for blk_a, blk_b in zip(a[:2], b[:2]):
        assert set(blk_a) == set(blk_b)
        tensors = [k for k, v in blk_a.items() if isinstance(v, torch.Tensor)]
        assert ("regionFullMean" if assemble else "fragFullMean") in tensors
        for k in tensors:
            va, vb = blk_a[k], blk_b[k]
            assert va.dtype == vb.dtype and va.shape == vb.shape, k
            if va.dtype == torch.float64:
                assert cti.same_bits(va.cpu().numpy(), vb.cpu().numpy()), k
            else:
                assert torch.equal(va, vb), k
        assert not torch.isnan(blk_a["regionFullMean" if assemble else "fragFullMean"]).all()
    assert a[2].equals(b[2])
