"""The region stage of the device (ru_count_kernel, ru_fill_kernel, ct_keys_kernel and its sort, count_join_kernel,
count_join_multi_kernel, count_join_inner_kernel, region_avdist_kernel) against tests/region_twin.py, a restatement of chicdiff.R in
Python integers, dicts and fractions that shares no code with the device path or with oracle/, on the small cases of
tests/region_inputs.py with the edges planted (tests/test_region_twin.py shows that each case reaches its edge, and holds the CPU
oracle to the same twin).

Every comparison is by equality, for float64 by bits with NaN in the same places: no tolerance anywhere.

The universe cases carry peaks with IDs at both ends of int32 as ordinary rows.  The window of such a peak does not fit 32 bits; the
kernels take it from ru_window.h (64-bit, clamped to the map), which tests/test_region_twin.py checks on its own first.
"""
import ctypes as C

import numpy as np
import pytest

import region_inputs as ri
import region_twin as rt
from post_inputs import region_universe_literal
from test_gpu_norm import ctx  # noqa: F401  (the module-scoped context fixture)
from test_region_twin import RU_KEYS, same_bits

pytestmark = pytest.mark.gpu

GUARD = 4096            # int32 words behind every output of the exact-capacity call
PATTERN = 0x5A5A5A5A
_TWINS = {}


def universe_twin(c):
    """computed once per case, shared by the tests, never written to"""
    key = id(c)
    if key not in _TWINS:
        _TWINS[key] = (c, rt.region_universe(c["bait"], c["oe"], c["s"], c["chr_of"]))
    return _TWINS[key][1]


def dev(ctx, a, dtype=None):
    return ctx.torch.from_numpy(np.ascontiguousarray(a, dtype=dtype)).to(ctx.device)


def case_id(c):
    return f"n{len(c['bait'])}-s{c['s']}-" + "+".join(sorted(c["planted"]))[:40]


UNIVERSE = ri.universe_cases()


@pytest.mark.parametrize("c", UNIVERSE, ids=case_id)
def test_region_universe_equals_the_twin(ctx, c):
    """HipContext.region_universe, the two-call path and the one call with exactly the required capacity, on every case."""
    torch = ctx.torch
    t = universe_twin(c)
    n, s, maxfrag = len(c["bait"]), c["s"], len(c["chr_of"]) - 1
    db, do, dc = dev(ctx, c["bait"]), dev(ctx, c["oe"]), dev(ctx, c["chr_of"])
    got = ctx.region_universe(db, do, s, dc)
    for k in RU_KEYS:
        assert np.array_equal(got[k].cpu().numpy(), t[k]), k
    total_exp = int(t["region_ptr"][-1])

    # count, then fill: no mask handed over, the fill forms the windows and the masks again
    ptr = torch.empty(n + 1, dtype=torch.int64, device=ctx.device)
    mn, mx = (torch.empty(n, dtype=torch.int32, device=ctx.device) for _ in range(2))
    total = C.c_int64(-1)
    ctx._check(ctx.lib.chicdiff_hip_region_universe_count_dev(ctx.h, db.data_ptr(), do.data_ptr(), n, s, dc.data_ptr(), maxfrag, ptr.data_ptr(),
                                                             mn.data_ptr(), mx.data_ptr(), C.byref(total)))
    assert total.value == total_exp
    for k, a in (("region_ptr", ptr), ("minOE", mn), ("maxOE", mx)):
        assert np.array_equal(a.cpu().numpy(), t[k]), ("count", k)
    rows = [torch.full((total_exp + GUARD,), PATTERN, dtype=torch.int32, device=ctx.device) for _ in range(3)]
    ctx._check(ctx.lib.chicdiff_hip_region_universe_fill_dev(ctx.h, db.data_ptr(), do.data_ptr(), n, s, dc.data_ptr(), maxfrag, ptr.data_ptr(),
                                                            *[r.data_ptr() for r in rows]))
    for k, r in zip(("baitID", "regionID", "otherEndID"), rows):
        r = r.cpu().numpy()
        assert np.array_equal(r[:total_exp], t[k]), ("count + fill", k)
        assert np.all(r[total_exp:] == PATTERN), ("count + fill wrote behind its rows", k)

    # the one call with exactly n * max(2 RUexpand + 1, 2) rows of room and a guard behind every output
    cap = n * max(2 * s + 1, 2)
    rows = [torch.full((cap + GUARD,), PATTERN, dtype=torch.int32, device=ctx.device) for _ in range(3)]
    ptr = torch.full((n + 1 + GUARD // 2,), PATTERN, dtype=torch.int64, device=ctx.device)
    mn, mx = (torch.full((n + GUARD,), PATTERN, dtype=torch.int32, device=ctx.device) for _ in range(2))
    total = C.c_int64(-1)
    ctx._check(ctx.lib.chicdiff_hip_region_universe_dev(ctx.h, db.data_ptr(), do.data_ptr(), n, s, dc.data_ptr(), maxfrag, ptr.data_ptr(), mn.data_ptr(),
                                                       mx.data_ptr(), *[r.data_ptr() for r in rows], cap, C.byref(total)))
    assert total.value == total_exp
    for k, a, used in (("region_ptr", ptr, n + 1), ("minOE", mn, n), ("maxOE", mx, n)):
        a = a.cpu().numpy()
        assert np.array_equal(a[:used], t[k]), ("exact capacity", k)
        assert np.all(a[used:] == PATTERN), ("guard touched", k)
    for k, r in zip(("baitID", "regionID", "otherEndID"), rows):
        r = r.cpu().numpy()
        assert np.array_equal(r[:total_exp], t[k]), ("exact capacity", k)
        assert np.all(r[cap:] == PATTERN), ("guard touched", k)
    with pytest.raises(Exception, match="rows needed"):
        bad = C.c_int64(0)
        ctx._check(ctx.lib.chicdiff_hip_region_universe_dev(ctx.h, db.data_ptr(), do.data_ptr(), n, s, dc.data_ptr(), maxfrag, ptr.data_ptr(), mn.data_ptr(),
                                                           mx.data_ptr(), *[r.data_ptr() for r in rows], cap - 1, C.byref(bad)))


def test_region_universe_grid_stride(ctx):
    """n = 4096 * 256 + 1 at RUexpand = 5: one region more than one pass of either launch covers; judged by the numpy form of the twin"""
    c = ri.universe_stride_case()
    t = rt.region_universe_np(c["bait"], c["oe"], c["s"], c["chr_of"])
    got = ctx.region_universe(dev(ctx, c["bait"]), dev(ctx, c["oe"]), c["s"], dev(ctx, c["chr_of"]))
    for k in RU_KEYS:
        assert np.array_equal(got[k].cpu().numpy(), t[k]), k
    assert t["region_ptr"][-1] > t["region_ptr"][-2]


@pytest.mark.parametrize("n,s", [(257, 5), (513, 16)])
def test_get_region_universe_mirror_is_the_literal_form(ctx, n, s):
    """post.getRegionUniverse returns RU.DT's own row order: region_universe_literal, row for row"""
    from chicdiff_amd import post
    c = ri.universe_case(n, s)
    ids = np.nonzero(c["chr_of"] >= 0)[0]
    ru = post.getRegionUniverse(ctx, c["bait"], c["oe"], s, c["chr_of"][ids].astype(str), ids)
    got = np.stack([ru[k].cpu().numpy() for k in ("baitID", "regionID", "otherEndID")], axis=1)
    assert np.array_equal(got, region_universe_literal(c["bait"], c["oe"], s, c["chr_of"]))
    t = universe_twin(c)
    for k in ("region_ptr", "minOE", "maxOE"):
        assert np.array_equal(ru[k].cpu().numpy(), t[k]), k


@pytest.mark.parametrize("case", ri.refusal_cases(), ids=lambda r: r[0])
def test_region_universe_refuses_bait_equal_oe_in_any_row(ctx, case):
    name, bait, oe, chr_of, s, row = case
    n, maxfrag = len(bait), len(chr_of) - 1
    db, do, dc = dev(ctx, bait), dev(ctx, oe), dev(ctx, chr_of)
    with pytest.raises(Exception, match="Invalid parameters"):
        ctx.region_universe(db, do, s, dc)
    ptr = ctx.torch.empty(n + 1, dtype=ctx.torch.int64, device=ctx.device)
    total = C.c_int64(0)
    with pytest.raises(Exception, match="Invalid parameters"):
        ctx._check(ctx.lib.chicdiff_hip_region_universe_count_dev(ctx.h, db.data_ptr(), do.data_ptr(), n, s, dc.data_ptr(), maxfrag, ptr.data_ptr(), None, None,
                                                                 C.byref(total)))


def test_region_universe_names_the_maxfrag_limit(ctx):
    """maxfrag >= 2^30 is refused before anything is read (the table here is the small one)"""
    c = ri.universe_case(255, 5)
    n = len(c["bait"])
    db, do, dc = dev(ctx, c["bait"]), dev(ctx, c["oe"]), dev(ctx, c["chr_of"])
    ptr = ctx.torch.empty(n + 1, dtype=ctx.torch.int64, device=ctx.device)
    rows = [ctx.torch.empty(11 * n, dtype=ctx.torch.int32, device=ctx.device) for _ in range(3)]
    total = C.c_int64(0)
    for maxfrag in (1 << 30, 2 ** 31 - 1):
        with pytest.raises(Exception, match=r"maxfrag < 2\^30"):
            ctx._check(ctx.lib.chicdiff_hip_region_universe_count_dev(ctx.h, db.data_ptr(), do.data_ptr(), n, 5, dc.data_ptr(), maxfrag, ptr.data_ptr(), None,
                                                                     None, C.byref(total)))
        with pytest.raises(Exception, match=r"maxfrag < 2\^30"):
            ctx._check(ctx.lib.chicdiff_hip_region_universe_fill_dev(ctx.h, db.data_ptr(), do.data_ptr(), n, 5, dc.data_ptr(), maxfrag, ptr.data_ptr(),
                                                                    *[r.data_ptr() for r in rows]))
        with pytest.raises(Exception, match=r"maxfrag < 2\^30"):
            ctx._check(ctx.lib.chicdiff_hip_region_universe_dev(ctx.h, db.data_ptr(), do.data_ptr(), n, 5, dc.data_ptr(), maxfrag, ptr.data_ptr(), None, None,
                                                               *[r.data_ptr() for r in rows], 11 * n, C.byref(total)))


# ---- key table ----------------------------------------------------------------------------------------------------------------
def device_key_table(ctx, c):
    flags = None if c["flags"] is None else dev(ctx, c["flags"], np.uint8)
    keys, vals = ctx.count_table(dev(ctx, c["bait"]), dev(ctx, c["oe"]), dev(ctx, c["N"]), flags)
    return keys.cpu().numpy(), vals.cpu().numpy()


@pytest.mark.parametrize("c", ri.key_table_cases() + [ri.key_table_repeats()],
                         ids=lambda c: f"rows{len(c['bait'])}-" + ("absent" if c["flags"] is None else "given" if c["flags"].any() else "zero"))
def test_count_table_equals_the_twin(ctx, c):
    """bait filter and stable sort; the repeated pairs of key_table_repeats stay in file order (nothing more is promised for them)"""
    keys, vals = device_key_table(ctx, c)
    ek, ev = rt.key_table(c["bait"], c["oe"], c["N"], c["flags"])
    assert np.array_equal(keys, ek) and np.array_equal(vals, ev)


def test_count_table_grid_stride(ctx):
    c = ri.key_table_case(ri.KEY_STRIDE_ROWS, "given")
    keys, vals = device_key_table(ctx, c)
    ek, ev = rt.key_table_np(c["bait"], c["oe"], c["N"], c["flags"])
    assert np.array_equal(keys, ek) and np.array_equal(vals, ev)


# ---- joins --------------------------------------------------------------------------------------------------------------------
def device_tables(ctx, c):
    return [(dev(ctx, k, np.int64), dev(ctx, v, np.int32)) for k, v in c["tables"]]


@pytest.mark.parametrize("c", ri.join_cases(), ids=lambda c: f"S{c['S']}-nru{len(c['qbait'])}-{c['variant']}")
def test_joins_equal_the_dict_twin(ctx, c):
    """count_join_inner against Reduce(merge) with dicts; count_join and count_join_multi against the plain dict look-up, on the same
    tables and queries"""
    qb, qo, tables = dev(ctx, c["qbait"]), dev(ctx, c["qoe"]), device_tables(ctx, c)
    inner = rt.join_inner(c["qbait"], c["qoe"], c["dicts"])                          # (nru, S)
    left = np.stack([rt.join_left(c["qbait"], c["qoe"], d) for d in c["dicts"]])     # (S, nru)
    assert np.array_equal(ctx.count_join_inner(qb, qo, tables).cpu().numpy(), inner.T)
    assert np.array_equal(ctx.count_join_multi(qb, qo, tables).cpu().numpy(), left)
    for t in sorted({0, c["S"] // 2, c["S"] - 1}):
        assert np.array_equal(ctx.count_join(qb, qo, *tables[t]).cpu().numpy(), left[t]), t


def test_joins_grid_stride(ctx):
    """nru = 8192 * 256 + 1 at S = 2: the rows of the small case drawn again and again, the twin's answers drawn with them"""
    c = ri.join_case(2, 257)
    idx = ri.tile_rows(257, ri.JOIN_STRIDE_NRU, 5)
    qb, qo, tables = dev(ctx, c["qbait"][idx]), dev(ctx, c["qoe"][idx]), device_tables(ctx, c)
    inner = rt.join_inner(c["qbait"], c["qoe"], c["dicts"])
    left = np.stack([rt.join_left(c["qbait"], c["qoe"], d) for d in c["dicts"]])
    assert inner.any() and not inner.all(axis=1).all()
    assert np.array_equal(ctx.count_join_inner(qb, qo, tables).cpu().numpy(), inner.T[:, idx])
    assert np.array_equal(ctx.count_join_multi(qb, qo, tables).cpu().numpy(), left[:, idx])


def test_count_join_inner_refuses_65_tables(ctx):
    c = ri.join_case(1, 255)
    qb, qo, tables = dev(ctx, c["qbait"]), dev(ctx, c["qoe"]), device_tables(ctx, c)
    with pytest.raises(Exception, match="count_join_inner"):
        ctx.count_join_inner(qb, qo, tables * 65)
    assert np.array_equal(ctx.count_join_inner(qb, qo, tables * 64).cpu().numpy()[63], rt.join_left(c["qbait"], c["qoe"], c["dicts"][0]))


# ---- avDist -------------------------------------------------------------------------------------------------------------------
def device_avdist(ctx, ru_bait, ru_oe, ptr, id_min, midsum, chr_codes):
    return ctx.region_avdist(dev(ctx, ru_bait, np.int32), dev(ctx, ru_oe, np.int32), dev(ctx, ptr, np.int64), id_min, dev(ctx, midsum, np.int64),
                             None if chr_codes is None else dev(ctx, chr_codes, np.int32)).cpu().numpy()


@pytest.mark.parametrize("c", ri.avdist_cases(), ids=lambda c: f"n{len(c['region_ptr']) - 1}-" + ("chr" if c["chr"] is not None else "nochr") + "-" + next(iter(c["planted"])))
def test_region_avdist_equals_the_twin_bit_for_bit(ctx, c):
    args = (c["ru_bait"], c["ru_oe"], c["region_ptr"], c["id_min"], c["midsum"], c["chr"])
    exp = rt.avdist(*args)
    got = device_avdist(ctx, *args)
    assert same_bits(got, exp), np.flatnonzero(~((got == exp) | (np.isnan(got) & np.isnan(exp))))[:10]


def test_region_avdist_grid_stride(ctx):
    """n = 4096 * 256 + 1 regions of one row each: the rows of a small case drawn again and again"""
    c = ri.avdist_case(257, True)
    m = len(c["ru_bait"])
    one = rt.avdist(c["ru_bait"], c["ru_oe"], np.arange(m + 1), c["id_min"], c["midsum"], c["chr"])     # every row as a region of its own
    assert np.isnan(one).any() and not np.isnan(one).all()
    idx = ri.tile_rows(m, ri.AVDIST_STRIDE_N, 9)
    got = device_avdist(ctx, c["ru_bait"][idx], c["ru_oe"][idx], np.arange(ri.AVDIST_STRIDE_N + 1), c["id_min"], c["midsum"], c["chr"])
    assert same_bits(got, one[idx])
