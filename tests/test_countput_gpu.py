"""countput on the device (HipContext.countput, pipeline.countput_dev) against the numpy twin of the rule in include/chicdiff_hip.h
(tests/countput_twin.py; tests/test_countput.py holds it equal to the pandas groupby of pipeline._countput): all six columns bit for
bit — NaN in the same cells, the same int64 views elsewhere — and the groups in the same order.  Tables: tests/countput_inputs.py."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import countput_inputs as cpi  # noqa: E402
from countput_twin import COLUMNS, countput_twin  # noqa: E402

gpu = pytest.mark.gpu
KEY_ROWS, REDUCE_ROWS = 1024, 256   # hip.countput_caps(), asserted below: the shapes around them are parametrised


@pytest.fixture(scope="module")
def ctx():
    import __graft_entry__ as g
    g.build()
    from chicdiff_amd import hip
    c = hip.HipContext(0)
    caps = hip.countput_caps()
    assert (caps["key_rows_per_workgroup"], caps["reduce_rows_per_workgroup"], caps["max_rep"]) == (KEY_ROWS, REDUCE_ROWS, 64)
    yield c
    c.close()


def upload(ctx, frames):
    torch = ctx.torch
    kinds = (np.int32, np.int32, np.int32, np.float64, np.float64, np.float64)
    return [tuple(torch.from_numpy(np.ascontiguousarray(x[name].to_numpy(), dtype=t)).to(ctx.device) for name, t in zip(COLUMNS, kinds))
            for x in frames]


def device_and_twin(ctx, frames, nid, tag):
    torch = ctx.torch
    midsum, chr_codes, _ = cpi.the_map(nid)
    want = countput_twin(frames, cpi.ID_MIN, midsum, chr_codes)
    got = ctx.countput(upload(ctx, frames), cpi.ID_MIN, torch.from_numpy(midsum).to(ctx.device), torch.from_numpy(chr_codes).to(ctx.device))
    assert list(got) == ["baitID", "otherEndID", "Nav", "Bav", "score", "oeID_mid"], tag
    got = {k: v.cpu().numpy() for k, v in got.items()}
    for k in ("baitID", "otherEndID"):
        assert got[k].dtype == np.int32 and np.array_equal(got[k], want[k]), (tag, k)
    for k in cpi.FLOAT_COLUMNS:
        assert got[k].dtype == np.float64 and cpi.same_bits(got[k], want[k]), (tag, k)
    return got


SIZES = [1, 64, 65, REDUCE_ROWS - 1, REDUCE_ROWS, REDUCE_ROWS + 1, KEY_ROWS - 1, KEY_ROWS, KEY_ROWS + 1, 20011]


@gpu
@pytest.mark.parametrize("total", SIZES)
def test_equal_to_the_twin_at_every_size(ctx, total):
    """One row, one wave, one row more; one row fewer than, exactly and one row more than a workgroup of the reduce pass and of the
    key pass takes; several workgroups.  1 to 4 replicates, with and without pairs repeated inside a replicate."""
    nrep = 1 if total < 64 else 1 + SIZES.index(total) % 4
    for dups in (False, True):
        frames, nid = cpi.condition(tuple(cpi.split(total, nrep)), 1 + SIZES.index(total), "shuffled", dups)
        assert sum(len(x) for x in frames) == total
        got = device_and_twin(ctx, frames, nid, (total, nrep, dups))
        assert total < 64 or 0 < len(got["Nav"]) < total


@gpu
@pytest.mark.parametrize("nrep", [1, 2, 3, 4])
@pytest.mark.parametrize("order", cpi.ORDERS)
def test_replicates_of_different_length_in_every_row_order(ctx, nrep, order):
    lengths = tuple(cpi.split(4097, nrep))
    assert len(set(lengths)) == nrep
    for dups in (False, True):
        frames, nid = cpi.condition(lengths, 20 + nrep, order, dups)
        got = device_and_twin(ctx, frames, nid, (nrep, order, dups))
        assert np.isnan(got["Bav"]).any() and np.isinf(got["Bav"]).any() and np.isnan(got["score"]).any()


@gpu
def test_a_replicate_without_rows_among_others(ctx):
    frames, nid = cpi.condition((300, 0, 65, 0), 5)
    assert [len(x) for x in frames] == [300, 0, 65, 0]
    a = device_and_twin(ctx, frames, nid, "empty replicates")
    b = device_and_twin(ctx, [frames[0], frames[2]], nid, "without them")
    for k in a:
        assert cpi.same_bits(a[k], b[k]), k


@gpu
def test_every_row_dropped_gives_no_group(ctx):
    frames, nid = cpi.condition((300, 65), 6)
    dropped = [x.assign(distSign=np.nan) for x in frames]
    got = device_and_twin(ctx, dropped, nid, "every distSign NaN")
    assert all(len(v) == 0 for v in got.values())
    off = [x.assign(otherEndID=np.int32(cpi.ID_MIN + nid // 3 + 2)) for x in frames]      # every other end in the map's gap
    assert all(len(v) == 0 for v in device_and_twin(ctx, off, nid, "every other end off the map").values())
    got = device_and_twin(ctx, [frames[0].iloc[:0], frames[1].iloc[:0]], nid, "no rows at all")
    assert all(len(v) == 0 for v in got.values())


@gpu
@pytest.mark.parametrize("scattered", [False, True], ids=["contiguous", "scattered"])
def test_one_pair_repeated_5000_times(ctx, scattered):
    """The group spans some twenty workgroups of the reduce pass in the sorted order and is walked by one lane."""
    frames, nid = cpi.repeated_pair(scattered)
    got = device_and_twin(ctx, frames, nid, ("repeated pair", scattered))
    k = np.flatnonzero((got["baitID"] == cpi.REP_BAIT) & (got["otherEndID"] == cpi.REP_OE))
    assert len(k) == 1
    rows = frames[0][(frames[0]["baitID"] == cpi.REP_BAIT) & frames[0]["distSign"].notna()]
    assert len(rows) > 4000 and rows["Bmean"].isna().any() and np.isinf(rows["Bmean"]).any()
    assert (rows.index[-1] - rows.index[0] > 20000) == scattered


@gpu
def test_first_appearance_in_the_last_row(ctx):
    import pandas as pd
    frames, nid = cpi.condition((1500, 1025), 7)
    last = cpi.values([cpi.REP_BAIT], [cpi.REP_OE], np.random.default_rng(0), na=0.0)
    frames = [frames[0], pd.concat([frames[1], last], ignore_index=True)]
    got = device_and_twin(ctx, frames, nid, "last row")
    assert got["baitID"][-1] == cpi.REP_BAIT and got["otherEndID"][-1] == cpi.REP_OE and (got["baitID"][:-1] != cpi.REP_BAIT).all()
    assert cpi.same_bits(got["Nav"][-1:], last["N"].to_numpy(np.float64)) and cpi.same_bits(got["Bav"][-1:], last["Bmean"].to_numpy())


@gpu
def test_hand_written_groups(ctx):
    """+-inf, inf - inf, signed zeros in both orders, groups without values, a pair repeated inside a replicate."""
    frames, nid = cpi.condition((300, 129, 65), 3)
    xs, expected = cpi.with_edges(list(frames), nid)
    got = device_and_twin(ctx, xs, nid, "edges")
    for k, (nav, bav, score) in enumerate(expected):
        at = np.flatnonzero(got["baitID"] == cpi.ID_MIN + nid + 100 + k)
        assert len(at) == 1, k
        for name, v in (("Nav", nav), ("Bav", bav), ("score", score)):
            assert cpi.same_bits(got[name][at], [v]), (k, name, got[name][at], v)


@gpu
def test_refusals_name_the_limit(ctx):
    from chicdiff_amd import hip
    torch = ctx.torch
    i = lambda n: torch.zeros(n, dtype=torch.int32, device=ctx.device)
    f = lambda n: torch.zeros(n, dtype=torch.float64, device=ctx.device)
    rep = lambda n=8: (i(n), i(n), i(n), f(n), f(n), f(n))
    d_midsum, d_chr = torch.zeros(16, dtype=torch.int64, device=ctx.device), i(16)
    with pytest.raises(ValueError, match="64"):
        ctx.countput([rep()] * 65, 0, d_midsum, d_chr)
    with pytest.raises(ValueError, match="64"):
        ctx.countput([], 0, d_midsum, d_chr)
    with pytest.raises(ValueError, match="empty restriction map"):
        ctx.countput([rep()], 0, d_midsum[:0], d_chr[:0])
    with pytest.raises(ValueError, match="shape"):
        ctx.countput([(i(8), i(8), i(8), f(8), f(7), f(8))], 0, d_midsum, d_chr)
    with pytest.raises(ValueError, match="dtype"):
        ctx.countput([(i(8), i(8), f(8), f(8), f(8), f(8))], 0, d_midsum, d_chr)
    with pytest.raises(hip.ChicdiffHipError, match="2147483647"):       # the map may not reach INT32_MAX: refused by the library
        ctx.countput([rep()], 2 ** 31 - 16, d_midsum, d_chr)

    def raw(nrep, nrows, nid=16):                                        # the library's own refusals: no row is read
        cols = rep()
        ptrs = [(C.c_void_p * max(nrep, 1))(*[t.data_ptr()] * max(nrep, 1)) for t in cols]
        out = [i(8).data_ptr()] * 2 + [f(8).data_ptr()] * 4
        g = C.c_int64(-1)
        rc = ctx.lib.chicdiff_hip_countput_dev(ctx.h, nrep, *ptrs, (C.c_int64 * len(nrows))(*nrows), 0, nid, d_midsum.data_ptr(), d_chr.data_ptr(),
                                               *out, C.byref(g))
        return rc, ctx.lib.chicdiff_hip_last_error(ctx.h), g.value
    for nrep in (0, 65):
        rc, msg, g = raw(nrep, [8] * max(nrep, 1))
        assert rc != 0 and b"nrep <= 64" in msg and g == 0, msg
    rc, msg, _ = raw(1, [8], nid=0)
    assert rc != 0 and b"nid = 0" in msg, msg
    rc, msg, _ = raw(2, [8, -1])
    assert rc != 0 and b"nrows[1] = -1" in msg, msg
    rc, msg, _ = raw(2, [2 ** 30, 2 ** 30])
    assert rc != 0 and b"2^31" in msg, msg
    rc, msg, g = raw(2, [0, 0])                                          # no rows: fine, no group
    assert rc == 0 and g == 0
    got = ctx.countput([rep()], 0, d_midsum, d_chr)                      # ... and a good call goes through: 8 rows of the pair (0, 0)
    assert len(got["Nav"]) == 1 and got["Nav"].item() == 0.0 and got["oeID_mid"].item() == 0.0


@pytest.fixture(scope="module")
def experiments(tmp_path_factory):
    from pipeline_inputs import make_experiment
    return {w: make_experiment(tmp_path_factory.mktemp("chin" if w else "nochin"), npeaks=1200, with_chinput=w)[0] for w in (True, False)}


@gpu
@pytest.mark.parametrize("with_chinput,device_tables", [(True, False), (False, False), (False, True)],
                         ids=["chinput", "no-chinput", "no-chinput-device-tables"])
def test_mirror_device_countput_same_frame(ctx, experiments, with_chinput, device_tables):
    """getFullRegionData(device_countput=True): the countput frame equals the pandas one bit for bit, in columns, dtypes and row order
    (also when the ID columns were uploaded once for the background tables), and both region blocks are unchanged."""
    import torch
    from chicdiff_amd import pipeline
    from pipeline_inputs import read_chicago_pickle
    settings = experiments[with_chinput]
    RU = pipeline.getRegionUniverse(settings, ctx)
    RUc = pipeline.getControlRegionUniverse(settings, RU, ctx, rng=np.random.default_rng(11))
    a = pipeline.getFullRegionData(settings, RU, RUc, ctx=ctx, read_chicago=read_chicago_pickle, device_tables=device_tables)
    b = pipeline.getFullRegionData(settings, RU, RUc, ctx=ctx, read_chicago=read_chicago_pickle, device_tables=device_tables, device_countput=True)
    cpi.assert_same_frame(b[2], a[2], "countput")
    assert len(a[2]) > 1000 and list(a[2]["condition"].unique()) == ["CD4", "Mono"] and a[2]["Bav"].isna().any()
    for blk_a, blk_b in zip(a[:2], b[:2]):
        assert set(blk_a) == set(blk_b)
        for k, va in blk_a.items():
            if not isinstance(va, torch.Tensor):
                continue
            vb = blk_b[k]
            assert va.dtype == vb.dtype and va.shape == vb.shape, k
            if va.dtype == torch.float64:
                assert cpi.same_bits(va.cpu().numpy(), vb.cpu().numpy()), k
            else:
                assert torch.equal(va, vb), k
