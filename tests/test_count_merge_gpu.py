"""chicdiff_hip_count_tables_merge_dev on the device (count_merge_mark_kernel, the scan, count_merge_write_kernel): the merged tables
against Reduce(merge) of tests/region_twin.py — keys, all S value columns and n_out —, then what is built on them: count_join_multi
and region_assemble on the merged tables against count_join_inner (-> fragment_background -> window_sums) on the original ones, and
the mirror's ``merge_counts=True`` against its default.

Every comparison is an equality: int32 and int64 by value, float64 by bits with NaN in the same places.  No tolerance, no rows left
out."""
import ctypes as C

import numpy as np
import pytest

import region_inputs as ri
import region_twin as rt
from test_count_merge import merged_tables
from test_region_assemble import assert_same

pytestmark = pytest.mark.gpu

INT32_MIN, INT32_MAX = -2 ** 31, 2 ** 31 - 1
GUARD = 4096            # int32 words behind every output of the exact-capacity call
PATTERN = 0x5A5A5A5A
PATTERN64 = (PATTERN << 32) | PATTERN
EDGE_VALUES = (INT32_MIN, -1, 0, INT32_MAX)


@pytest.fixture(scope="module")
def ctx():
    import __graft_entry__ as g
    g.build()
    from chicdiff_amd import hip
    c = hip.HipContext(0)
    yield c
    c.close()


def dev(ctx, a, dtype=None):
    return ctx.torch.from_numpy(np.ascontiguousarray(a, dtype=dtype)).to(ctx.device)


def device_tables(ctx, tables):
    return [(dev(ctx, k, np.int64), dev(ctx, v, np.int32)) for k, v in tables]


def twin(tables):
    """Reduce(merge) of (keys, vals) numpy tables by the dict twin -> (keys, vals (S, n))."""
    keys, vals, _ = merged_tables([rt.table_dict(k, v) for k, v in tables])
    return keys, vals


def check(ctx, tables, want=None, tag=""):
    """``merge_count_tables`` on ``tables`` (numpy) against the twin: keys, every value column, n_out; the binding's promises."""
    keys, vals = twin(tables) if want is None else want
    got = ctx.merge_count_tables(device_tables(ctx, tables))
    assert len(got) == len(tables), tag
    assert all(k is got[0][0] for k, _ in got), (tag, "one keys tensor for all replicates")
    gk = got[0][0].cpu().numpy()
    assert gk.dtype == np.int64 and gk.shape == keys.shape and np.array_equal(gk, keys), (tag, "keys / n_out", gk.shape, keys.shape)
    for s, (_, v) in enumerate(got):
        assert v.is_contiguous() and v.dtype == ctx.torch.int32 and v.shape == (len(keys),), (tag, s)
        assert np.array_equal(v.cpu().numpy(), vals[s]), (tag, "values of table", s)
    return got


def pack_pairs(b, o):
    return (np.asarray(b, dtype=np.int64) << 32) | (np.asarray(o, dtype=np.int64) & 0xFFFFFFFF)


def key_universe(rng, m):
    """m distinct keys, ascending: baits negative, 0, ordinary and INT32_MAX, other ends over all of int32 with both ends planted."""
    b = np.concatenate([rng.integers(1, 60, m), [INT32_MIN, -7, -1, 0, 0, INT32_MAX, INT32_MAX, INT32_MAX, 5, 5]])
    o = np.concatenate([rng.integers(-300, 3000, m), [0, INT32_MAX, INT32_MIN, INT32_MIN, INT32_MAX, INT32_MIN, INT32_MAX, 0, INT32_MIN, INT32_MAX]])
    return np.unique(pack_pairs(b, o))


def values(rng, n):
    v = rng.integers(-50, 500, n).astype(np.int32)
    at = rng.integers(0, max(n, 1), min(n, 8 * len(EDGE_VALUES)))
    v[at] = np.resize(np.array(EDGE_VALUES, dtype=np.int32), len(at))
    return v


def subset(rng, u, size):
    return np.sort(rng.choice(u, size=size, replace=False))


# ---- the merge against the twin ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("c", ri.join_cases(), ids=lambda c: f"S{c['S']}-nru{len(c['qbait'])}-{c['variant']}")
def test_merge_equals_reduce_merge_on_the_join_cases_in_every_rotation(ctx, c):
    """S = 1, 2, 3, 8, 64, one table empty, one-key tables; the list rotated, so that the pivot (the smallest table, the first of them
    on a tie) sits in another place — for the one-key tables and S = 1 it is another table: same keys, the columns rotated with it."""
    S = c["S"]
    keys, vals, merged = merged_tables(c["dicts"])
    if c["variant"] == "normal" and S > 1:
        assert 0 < len(keys) < min(len(k) for k, _ in c["tables"])
        at = int(np.searchsorted(keys, rt.pack(10, 300)))
        assert keys[at] == rt.pack(10, 300) and vals[0, at] == 0      # "zero_hit" is held
    if c["variant"] == "one_empty":
        assert len(keys) == 0
    for r in sorted({0, 1 % S, S // 2, S - 1}):
        tables = c["tables"][r:] + c["tables"][:r]
        check(ctx, tables, (keys, np.roll(vals, -r, axis=0)), ("rotation", r))


@pytest.mark.parametrize("S", (2, 16, 17, 33))
@pytest.mark.parametrize("npivot", (0, 1, 511, 512, 513, 1025, 2049))
def test_pivot_sizes_and_table_counts(ctx, npivot, S):
    """The pivot has 0, 1, 511, 512, 513 (a last, partial tile), 1 025 and 2 049 (more than one workgroup) keys, among S - 1 larger
    tables: 17 = one full batch of other tables, 33 = the mask carried over two batch borders.  Keys over all of int32 x int32, values
    with the int32 ends; the pivot in the first, a middle and the last place."""
    rng = np.random.default_rng(1000 * S + npivot)
    u = key_universe(rng, 4000)
    core = subset(rng, u, 300)                                         # held by every larger table: the result is not empty
    for place in sorted({0, S // 3, S - 1}):
        tables = []
        for s in range(S):
            k = subset(rng, u, npivot) if s == place else np.union1d(core, subset(rng, u, int(rng.integers(2100, 3600))))
            tables.append((k, values(rng, len(k))))
        got = check(ctx, tables, tag=(npivot, S, place))
        assert npivot == 0 or got[0][0].numel() > 0 or npivot == 1


def test_table_shapes(ctx):
    rng = np.random.default_rng(77)
    u = key_universe(rng, 3000)
    for S in (1, 2, 5, 18):
        # identical key sets: the identity, whichever table is the pivot (a tie: the first)
        k = subset(rng, u, 1300)
        tables = [(k, values(rng, len(k))) for _ in range(S)]
        got = check(ctx, tables, (k, np.stack([v for _, v in tables])), ("identity", S))
        assert got[0][0].numel() == 1300
        if S == 1:
            continue
        # disjoint tables: nothing is kept, whatever the order
        parts = np.array_split(rng.permutation(u[: 600 * S]), S)
        tables = [(np.sort(p), values(rng, len(p))) for p in parts]
        assert check(ctx, tables, tag=("disjoint", S))[0][0].numel() == 0
        assert check(ctx, tables[::-1], tag=("disjoint, reversed", S))[0][0].numel() == 0
        # the only common key is the pivot's first / last key
        for which in ("first", "last"):
            only = u[0] if which == "first" else u[-1]
            inner = u[1:-1]
            parts = np.array_split(rng.permutation(inner[: 700 * S]), S)
            tables = [(np.sort(np.append(p[: max(len(p) - 5 * s, 1)], only)), None) for s, p in enumerate(parts)]
            tables = [(k, values(rng, len(k))) for k, _ in tables]
            for order in (tables, tables[::-1]):                       # the pivot (the shortest: the last part) last and first
                got = check(ctx, order, tag=(which, S))
                assert got[0][0].cpu().tolist() == [int(only)]


@pytest.mark.parametrize("S", (2, 3))
def test_sparse_pivot_over_a_dense_table_takes_the_global_search(ctx, S):
    """512 pivot keys spread over a 70 001-key table: the tile's range holds far more than 768 keys (the search in global memory);
    and the reverse order of the list.  Half of the pivot's keys are in the dense table."""
    rng = np.random.default_rng(5 + S)
    dense = np.unique(pack_pairs(rng.integers(-3, 400, 90000), rng.integers(-2000, 2000, 90000)))[:70001]
    assert len(dense) == 70001
    outside = np.setdiff1d(pack_pairs(rng.integers(-3, 400, 600), rng.integers(2000, 4000, 600)), dense)[:256]
    pivot = np.union1d(dense[rng.choice(70001, 256, replace=False)], outside)
    assert len(pivot) == 512
    tables = [(pivot, values(rng, 512)), (dense, values(rng, 70001))]
    if S == 3:
        tables.append((np.union1d(pivot[::2], dense[::3]), None))
        tables[2] = (tables[2][0], values(rng, len(tables[2][0])))
    for order in (tables, tables[::-1]):
        got = check(ctx, order, tag=("sparse over dense", S))
        assert got[0][0].numel() == 256 if S == 2 else 0 < got[0][0].numel() < 256


def test_key_ranges_and_values_come_back_unchanged(ctx):
    pairs = [(INT32_MIN, INT32_MIN), (INT32_MIN, INT32_MAX), (-1, -1), (-1, 0), (0, INT32_MIN), (0, -1), (0, 0), (0, INT32_MAX), (7, 3),
             (INT32_MAX, INT32_MIN), (INT32_MAX, 0), (INT32_MAX, INT32_MAX)]
    keys = np.array(sorted(rt.pack(b, o) for b, o in pairs), dtype=np.int64)
    v0 = np.resize(np.array(EDGE_VALUES, dtype=np.int32), len(keys))
    v1 = np.resize(np.array(EDGE_VALUES[::-1], dtype=np.int32), len(keys))
    more = np.union1d(keys, np.array([rt.pack(3, 3), rt.pack(-5, 9)], dtype=np.int64))
    v2 = np.arange(len(more), dtype=np.int32) - 4
    got = check(ctx, [(keys, v0), (more, v2), (keys, v1)])
    assert got[0][0].numel() == len(keys)
    assert got[0][1].cpu().tolist() == v0.tolist() and got[2][1].cpu().tolist() == v1.tolist()


def raw_call(ctx, tables_dev, S, cap, keys_out, vals_out):
    """The entry point itself -> (return code, n_out)."""
    n = len(tables_dev)
    kp, vp, nk = (C.c_void_p * max(n, 1))(), (C.c_void_p * max(n, 1))(), (C.c_int64 * max(n, 1))()
    for s, (k, v) in enumerate(tables_dev):
        kp[s], vp[s], nk[s] = k.data_ptr(), v.data_ptr(), k.numel()
    n_out = C.c_int64(-1)
    rc = ctx.lib.chicdiff_hip_count_tables_merge_dev(ctx.h, S, kp, vp, nk, cap, keys_out.data_ptr(), vals_out.data_ptr(), C.byref(n_out))
    return rc, n_out.value


def test_exact_capacity_guards_refusals_and_repeats(ctx):
    torch = ctx.torch
    c = ri.join_case(8, 257)
    keys, vals, _ = merged_tables(c["dicts"])
    tables = device_tables(ctx, c["tables"])
    S, cap, n = 8, min(len(k) for k, _ in c["tables"]), len(keys)
    assert 0 < n < cap

    def fresh():
        return (torch.full((cap + GUARD // 2,), PATTERN64, dtype=torch.int64, device=ctx.device),
                torch.full((S * cap + GUARD,), PATTERN, dtype=torch.int32, device=ctx.device))

    # cap exactly min nkeys: the rows, and nothing behind them — neither behind n_out inside a column nor behind the outputs
    ko, vo = fresh()
    rc, n_out = raw_call(ctx, tables, S, cap, ko, vo)
    assert rc == 0 and n_out == n
    k, v = ko.cpu().numpy(), vo.cpu().numpy()
    assert np.array_equal(k[:n], keys) and np.all(k[n:] == PATTERN64), "keys / guard touched"
    cols = v[: S * cap].reshape(S, cap)
    assert np.array_equal(cols[:, :n], vals) and np.all(cols[:, n:] == PATTERN) and np.all(v[S * cap:] == PATTERN), "values / guard touched"
    # the same bits on a repeated call, into the same buffers and through the binding
    rc, n_out = raw_call(ctx, tables, S, cap, ko, vo)
    assert rc == 0 and n_out == n and np.array_equal(ko.cpu().numpy(), k) and np.array_equal(vo.cpu().numpy(), v)
    a, b = ctx.merge_count_tables(tables), ctx.merge_count_tables(tables)
    assert torch.equal(a[0][0], b[0][0]) and all(torch.equal(x[1], y[1]) for x, y in zip(a, b))
    # cap one short: refused, nothing written
    ko, vo = fresh()
    rc, _ = raw_call(ctx, tables, S, cap - 1, ko, vo)
    assert rc != 0 and "rows needed" in ctx.lib.chicdiff_hip_last_error(ctx.h).decode()
    assert bool((ko == PATTERN64).all()) and bool((vo == PATTERN).all())
    # S = 0 and S = 65: refused by the entry point and by the binding
    for bad in (0, 65):
        rc, _ = raw_call(ctx, (tables * 9)[:bad], bad, cap, ko, vo)
        assert rc != 0 and "S" in ctx.lib.chicdiff_hip_last_error(ctx.h).decode(), bad
        with pytest.raises(ValueError, match="64"):
            ctx.merge_count_tables((tables * 9)[:bad])
    assert bool((ko == PATTERN64).all()) and bool((vo == PATTERN).all())
    assert len(ctx.merge_count_tables((tables * 8)[:64])) == 64        # 64 is served
    # a NULL output
    n_out = C.c_int64(0)
    kp, vp, nk = (C.c_void_p * 1)(tables[0][0].data_ptr()), (C.c_void_p * 1)(tables[0][1].data_ptr()), (C.c_int64 * 1)(tables[0][0].numel())
    assert ctx.lib.chicdiff_hip_count_tables_merge_dev(ctx.h, 1, kp, vp, nk, nk[0], None, vo.data_ptr(), C.byref(n_out)) != 0
    assert ctx.lib.chicdiff_hip_count_tables_merge_dev(ctx.h, 1, kp, vp, nk, nk[0], ko.data_ptr(), vo.data_ptr(), None) != 0
    assert ctx.lib.chicdiff_hip_count_tables_merge_dev(ctx.h, 1, None, vp, nk, nk[0], ko.data_ptr(), vo.data_ptr(), C.byref(n_out)) != 0


def test_binding_refuses_bad_tables(ctx):
    torch = ctx.torch
    c = ri.join_case(3, 255)
    tables = device_tables(ctx, c["tables"])
    k0, v0 = tables[0]
    wide = torch.zeros(2 * k0.numel(), dtype=torch.int64, device=ctx.device)[::2]
    assert wide.numel() == k0.numel() and not wide.is_contiguous()
    for tag, bad in (("dtype of keys", [(k0.to(torch.int32), v0)] + tables[1:]),
                     ("dtype of vals", [(k0, v0.to(torch.int64))] + tables[1:]),
                     ("non-contiguous keys", [(wide, v0)] + tables[1:]),
                     ("non-contiguous vals", tables[:2] + [(tables[2][0], torch.zeros(2 * tables[2][0].numel(), dtype=torch.int32, device=ctx.device)[::2])]),
                     ("keys != vals", [(k0, v0[:-1])] + tables[1:]),
                     ("a CPU table", [(k0.cpu(), v0.cpu())] + tables[1:]),
                     ("not pairs", [k0, v0])):
        with pytest.raises(ValueError):
            ctx.merge_count_tables(bad)
            pytest.fail(tag)
    check(ctx, c["tables"])


def test_refusal_comes_before_the_entry_point(ctx):
    """The row of tests/test_binding_refusals_gpu.py for this method, on that file's inputs and table cases: with every entry point
    walled off a good call reaches the library, a bad table is refused before it, and the message names the table."""
    from test_binding_refusals_gpu import Inputs, NoLaunch, Reached, table_cases
    v = Inputs(ctx)
    lib = ctx.lib
    ctx.lib = NoLaunch(lib)
    try:
        with pytest.raises(Reached):
            ctx.merge_count_tables(v.tables)
        cases = table_cases(v)
        assert cases
        for tag, who, change in cases:
            with pytest.raises(ValueError) as e:
                ctx.merge_count_tables(change["tables"])
            assert who in str(e.value), (tag, str(e.value))
    finally:
        ctx.lib = lib
    assert len(ctx.merge_count_tables(v.tables)) == len(v.tables)


# ---- downstream ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("c", ri.join_cases(), ids=lambda c: f"S{c['S']}-nru{len(c['qbait'])}-{c['variant']}")
def test_count_join_multi_on_the_merged_tables_is_count_join_inner(ctx, c):
    qb, qo, tables = dev(ctx, c["qbait"]), dev(ctx, c["qoe"]), device_tables(ctx, c["tables"])
    inner = ctx.count_join_inner(qb, qo, tables)
    assert np.array_equal(inner.cpu().numpy(), rt.join_inner(c["qbait"], c["qoe"], c["dicts"]).T)
    got = ctx.count_join_multi(qb, qo, ctx.merge_count_tables(tables))
    assert got.dtype == inner.dtype and got.shape == inner.shape and ctx.torch.equal(got, inner)


@pytest.mark.parametrize("S", (1, 8, 17))
@pytest.mark.parametrize("n", (1, 45, 46, 47, 257))
def test_region_assemble_on_the_merged_tables_is_the_inner_path(ctx, n, S):
    """region_assemble(merged) against count_join_inner -> fragment_background(only_fullmean=True) -> window_sums on the inputs of
    tests/assemble_inputs.py, pairs dropped from the first, a middle and the last replicate; n regions on both sides of the 46-region
    tile; the tile path and the generic one."""
    from assemble_inputs import assemble, background_args, make
    torch = ctx.torch
    d = make(ctx, n, S, counts="device")
    bg = background_args(d)
    g = torch.Generator(device=ctx.device)
    g.manual_seed(100 * n + S)
    tables = list(d["tables"])
    for s in sorted({0, S // 2, S - 1}):
        ks, vs = tables[s]
        keep = torch.rand(ks.numel(), device=ctx.device, generator=g) < 0.7
        if ks.numel() > 1:
            keep[int(torch.randint(0, ks.numel(), (1,), generator=g, device=ctx.device))] = False
        tables[s] = (ks[keep].contiguous(), vs[keep].contiguous())
    fragN = ctx.count_join_inner(d["bait"], d["oe"], tables)
    _, _, fragFM = ctx.fragment_background(d["bait"], d["oe"], *bg, only_fullmean=True)
    ref = ctx.window_sums(fragN, fragFM, d["region_ptr"])
    if S > 1 and n > 1:
        assert not torch.equal(fragN, ctx.count_join_multi(d["bait"], d["oe"], tables))   # the inner join differs from the left join
    merged = ctx.merge_count_tables(tables)
    assert merged[0][0].numel() <= min(k.numel() for k, _ in tables)
    assert_same(assemble(ctx, d["bait"], d["oe"], d["region_ptr"], merged, bg), ref, (n, S, "tile"))
    ctx.set_option("region_assemble_generic", 1)
    try:
        assert_same(assemble(ctx, d["bait"], d["oe"], d["region_ptr"], merged, bg), ref, (n, S, "generic"))
    finally:
        ctx.set_option("region_assemble_generic", 0)


# ---- the mirror ------------------------------------------------------------------------------------------------------------------
def same_frame(got, ref, tag):
    assert list(got.columns) == list(ref.columns) and len(got) == len(ref) and got.attrs == ref.attrs, tag
    for col in ref.columns:
        a, b = got[col].to_numpy(), ref[col].to_numpy()
        if a.dtype == np.float64:
            nan = np.isnan(b)
            assert np.array_equal(np.isnan(a), nan) and np.array_equal(a.view(np.int64)[~nan], b.view(np.int64)[~nan]), (tag, col)
        else:
            assert a.dtype == b.dtype and np.array_equal(a, b), (tag, col)


def test_mirror_merge_counts_gives_the_default_blocks_and_fits(ctx, tmp_path, capsys):
    """getFullRegionData(merge_counts=True) against the default (count_join_inner per universe): the fragment blocks; then
    assemble=True with it -> DESeq2Wrap against the default path, every column, test and control set (check 4 of
    tests/test_region_assemble.py on the branch without chinput files)."""
    from chicdiff_amd import pipeline
    from pipeline_inputs import make_experiment, read_chicago_pickle
    torch = ctx.torch
    settings, _ = make_experiment(tmp_path, npeaks=2500, with_chinput=False)
    assert pipeline.asChicdiffSettings(settings)["countData"] is None
    RU = pipeline.getRegionUniverse(settings, ctx)
    RUc = pipeline.getControlRegionUniverse(settings, RU, ctx, rng=np.random.default_rng(11))
    frd = pipeline.getFullRegionData(settings, RU, RUc, ctx=ctx, read_chicago=read_chicago_pickle)
    capsys.readouterr()
    frd_m = pipeline.getFullRegionData(settings, RU, RUc, ctx=ctx, read_chicago=read_chicago_pickle, merge_counts=True)
    assert capsys.readouterr().err.count("Merging countData") == 1    # once, not per universe
    frd_a = pipeline.getFullRegionData(settings, RU, RUc, ctx=ctx, read_chicago=read_chicago_pickle, merge_counts=True, assemble=True)
    for blk, blk_m, blk_a in zip(frd[:2], frd_m[:2], frd_a[:2]):
        assert torch.equal(blk_m["fragN"], blk["fragN"]) and bool((blk["fragN"] > 0).any())
        assert_same((blk_m["fragN"], blk_m["fragFullMean"]), (blk["fragN"], blk["fragFullMean"]), "fragment block")
        assert torch.equal(blk_m["region_ptr"], blk["region_ptr"]) and torch.equal(blk_a["region_ptr"], blk["region_ptr"])
        for other in (blk_m, blk_a):
            assert torch.equal(other["avDist"].view(torch.int64), blk["avDist"].view(torch.int64)) and other["is_control"] == blk["is_control"]
        assert "fragN" not in blk_a
        assert_same((blk_a["regionN"], blk_a["regionFullMean"]), ctx.window_sums(blk["fragN"], blk["fragFullMean"], blk["region_ptr"]), "region block")
    for norm in ("standard", "fullmean", "combined"):
        st = dict(settings, norm=norm)
        theta = None
        for u, blk, blk_a, suffix in ((RU, frd[0], frd_a[0], ""), (RUc, frd[1], frd_a[1], "Control")):
            ref = pipeline.DESeq2Wrap(st, u, blk, suffix=suffix, theta=theta, ctx=ctx)
            got = pipeline.DESeq2Wrap(st, u, blk_a, suffix=suffix, theta=theta, ctx=ctx)
            assert len(ref) == blk["n"] and np.isfinite(ref["pvalue"].to_numpy()).any()
            same_frame(got, ref, (norm, suffix))
            theta = ref.attrs.get("theta")


def test_chicdiffPipeline_merge_counts_gives_the_same_result_table(ctx, tmp_path):
    from chicdiff_amd import pipeline
    from pipeline_inputs import make_experiment, quantile_ihw, read_chicago_pickle
    settings, _ = make_experiment(tmp_path, npeaks=1200, with_chinput=False)
    runs = []
    for name, kw in (("default", {}), ("merged", dict(merge_counts=True)), ("merged_assembled", dict(merge_counts=True, assemble=True))):
        st = dict(settings, outprefix=str(tmp_path / name))
        runs.append(pipeline.chicdiffPipeline(st, ctx=ctx, read_chicago=read_chicago_pickle, ihw=quantile_ihw(), rng=np.random.default_rng(11), **kw))
    assert len(runs[0]) > 100
    same_frame(runs[1], runs[0], "merge_counts")
    same_frame(runs[2], runs[0], "merge_counts + assemble")
