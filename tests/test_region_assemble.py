"""chicdiff_hip_region_assemble_dev: region-level N and FullMean in one kernel, held to BIT IDENTITY with the three calls it
replaces (count_join_multi -> fragment_background(only_fullmean=True) -> window_sums).  Every comparison is exact: the int32
matrix by equality, the fp64 matrix by its int64 view wherever it is not NaN (that covers every finite value and the
infinities) and NaN in the same places; no tolerance, no rows left out."""
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
gpu = pytest.mark.gpu


# ---- without a GPU ------------------------------------------------------------------------------------------------------------
def test_entry_point_is_declared_listed_and_exported():
    import __graft_entry__ as g
    g.build()
    from chicdiff_amd import hip
    sym = "chicdiff_hip_region_assemble_dev"
    hdr = open(os.path.join(ROOT, "include", "chicdiff_hip.h")).read()
    assert re.search(r"\bint\s+" + sym + r"\s*\(", hdr)
    for lines in ("843-858", "628-703", "894-896", "1540-1547"):      # the reference lines it replaces, cited in the header
        assert lines in hdr[hdr.index("a1 + a3 + a2"):hdr.index("int " + sym)], lines
    assert "bit for bit" in hdr[hdr.index("a1 + a3 + a2"):hdr.index("int " + sym)]
    assert sym in hip.EXPORTS and hasattr(hip.load_library(), sym)
    assert hasattr(hip.HipContext, "region_assemble")


def test_assemble_without_count_data_names_the_branch(tmp_path):
    """getFullRegionData(assemble=True) covers the chinput branch only: without countData it says so before it needs a device."""
    from chicdiff_amd import pipeline
    from pipeline_inputs import make_experiment
    settings, _ = make_experiment(tmp_path, npeaks=300, with_chinput=False)
    with pytest.raises(ValueError, match="chinput branch"):
        pipeline.getFullRegionData(settings, None, None, ctx=None, read_chicago=lambda p: None, assemble=True)
    import inspect
    assert inspect.signature(pipeline.getFullRegionData).parameters["assemble"].default is False
    assert inspect.signature(pipeline.chicdiffPipeline).parameters["assemble"].default is False


# ---- on the GPU ---------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def ctx():
    import __graft_entry__ as g
    g.build()
    from chicdiff_amd import hip
    c = hip.HipContext(0)
    yield c
    c.close()


def assert_same(got, ref, tag):
    import torch
    (N, FM), (Nr, FMr) = got, ref
    if Nr is not None:
        assert N.dtype == torch.int32 and N.shape == Nr.shape and torch.equal(N, Nr), (tag, "N", int((N != Nr).sum()))
    if FMr is not None:
        assert FM.dtype == torch.float64 and FM.shape == FMr.shape, tag
        nan = torch.isnan(FMr)
        assert torch.equal(torch.isnan(FM), nan), (tag, "NaN places")
        a, b = FM.view(torch.int64)[~nan], FMr.view(torch.int64)[~nan]
        assert torch.equal(a, b), (tag, "FullMean bits", int((a != b).sum()))


def cut_regions(rng, nrows, empty_share=0.1, lo=1, hi=11):
    """region_ptr over exactly ``nrows`` rows: random spans lo .. hi, a share of empty regions (first and last included)."""
    spans = [0]
    total = 0
    while total < nrows:
        s = 0 if rng.random() < empty_share else int(rng.integers(lo, hi + 1))
        s = min(s, nrows - total)
        spans.append(s)
        total += s
    spans.append(0)
    return np.concatenate([[0], np.cumsum(spans)]).astype(np.int64)


class Shapes:
    """The inputs of checks 1 and 2: the RU rows of tests/test_oracle.py::_a3_inputs (real chr19 geometry, FullMean with NaNs),
    repeated and kept in bait order, a few rows with IDs off the map / extreme; key tables from those rows' own pairs, thinned per
    replicate as test_count_join_all_replicates_in_one_pass thins them (dense / medium / sparse / EMPTY), plus keys that no row
    asks for — dense enough that tiles fall on both sides of the 768-key window."""

    def __init__(self, ctx, S):
        import torch
        from test_oracle import _a3_inputs
        self.ctx, self.S = ctx, S
        a = _a3_inputs(seed=5, S=S)
        rng = np.random.default_rng(4242 + S)
        t = lambda x: torch.as_tensor(np.ascontiguousarray(x)).to(ctx.device)
        rb, ro = np.tile(a["bait"], 7), np.tile(a["oe"], 7)
        xb = np.array([2 ** 31 - 1, a["id_min"] - 3, -5, a["id_min"] + 10, a["id_min"] + 5000, 0], dtype=np.int32)   # off the map / extreme
        xo = np.array([-1, a["id_min"] + 7, 7, 2 ** 31 - 1, a["id_min"] + 20, 0], dtype=np.int32)
        at = rng.integers(0, len(rb), len(xb))
        rb, ro = np.insert(rb, at, xb), np.insert(ro, at, xo)
        order = np.argsort(rb, kind="stable")                         # setkey(RU, baitID)
        self.rb, self.ro = rb[order].astype(np.int32), ro[order].astype(np.int32)
        own = np.unique((a["bait"].astype(np.int64) << 32) | a["oe"].astype(np.int64))
        baits = np.unique(a["bait"]).astype(np.int64)
        other = np.unique((np.repeat(baits, 700) << 32) | (np.repeat(baits, 700) + np.tile(np.arange(-350, 350), len(baits))))
        allk = np.union1d(own, other)
        self.tabs = []
        for s in range(S):
            kk = allk[rng.uniform(size=len(allk)) < (0.9, 0.5, 0.02, 0.0, 0.3)[s % 5]]
            self.tabs.append((t(kk), t(rng.integers(1, 500, len(kk)).astype(np.int32))))
        self.db, self.do = t(self.rb), t(self.ro)
        self.bg = (a["id_min"], t(a["midsum"]), t(a["sj"]), t(a["si"]), t(a["tblb"]), t(a["tlb"]), t(a["T"]), a["distfun"])
        self.rng = rng
        self.t = t

    def check(self, nq, off, ptr=None, tag=""):
        from assemble_inputs import assemble, three_calls
        db, do = self.db[off:nq], self.do[off:nq]                     # (off = 1, 3: pointers that are only 4-byte aligned)
        if ptr is None:
            ptr = cut_regions(self.rng, nq - off)
        assert ptr[-1] == nq - off
        dptr = self.t(ptr)
        ref = three_calls(self.ctx, db, do, dptr, self.tabs, self.bg)
        got = assemble(self.ctx, db, do, dptr, self.tabs, self.bg)
        assert_same(got, ref, (self.S, nq, off, tag))
        return got, ref, (db, do, dptr)


def run_shapes(ctx):
    import torch
    from assemble_inputs import assemble
    seen_nan = seen_counts = seen_empty = False
    for S in (1, 2, 3, 8, 16, 20):                                    # 20: two launches (16 tables per launch)
        sh = Shapes(ctx, S)
        full = len(sh.rb)
        assert full > 30001
        cases = [(full, 0), (full - 1, 0), (full - 2, 0), (full - 3, 0), (513, 0), (1, 0), (7, 0), (4099, 0), (30001, 1), (30001, 3),
                 (512, 0), (1024, 2)]
        if S in (3, 16):                                              # (the other replicate counts: a subset, to bound the run)
            cases = cases[:5] + cases[8:10]
        elif S != 8:
            cases = [cases[0], cases[3], cases[8]]
        for nq, off in cases:
            (N, FM), _, (db, do, dptr) = sh.check(nq, off)
            seen_nan |= bool(torch.isnan(FM).any())
            seen_counts |= bool((N > 0).any())
            seen_empty |= bool((dptr[1:] == dptr[:-1]).any())
            if (nq, off) in ((full, 0), (30001, 3)):                   # one output only: the other's inputs are not touched
                assert_same(assemble(ctx, db, do, dptr, sh.tabs, sh.bg, want_FullMean=False), (N, None), (S, nq, off, "N only"))
                assert_same(assemble(ctx, db, do, dptr, sh.tabs, sh.bg, want_N=False), (None, FM), (S, nq, off, "FullMean only"))
                assert assemble(ctx, db, do, dptr, sh.tabs, sh.bg, want_N=False)[0] is None
        # n = 1: one region holds all the rows (7 of them: the tile path; 600: the generic one)
        for rows in (7, 600):
            sh.check(rows, 0, ptr=np.array([0, rows], dtype=np.int64), tag="n = 1")
        # nru = 0: every region is empty.  (window_sums cannot be the reference here: its binding takes a matrix without rows for "not
        # asked for".)  0 / 0.0 is what window_sums_kernel gives an empty region.
        e = sh.db[:0]
        N, FM = assemble(ctx, e, e, sh.t(np.zeros(4, dtype=np.int64)), sh.tabs, sh.bg)
        assert N.shape == (S, 3) and FM.shape == (S, 3) and not N.any() and torch.equal(FM.view(torch.int64), torch.zeros_like(N, dtype=torch.int64))
    assert seen_nan and seen_counts and seen_empty                    # some region sums ARE NaN, some N > 0, some regions empty
    return True


@gpu
def test_bit_identity_with_the_three_calls_over_shapes(ctx):
    """Check 1: dense / medium / sparse / empty tables, S in {1, 2, 3, 8, 16, 20}, row counts in every residue mod 4, pointer
    offsets 1 and 3, IDs off the map and extreme, regions of 1 .. 11 rows with empty ones between, n = 1, nru = 0, one output only."""
    assert run_shapes(ctx)


@gpu
def test_generic_path_forced_on_every_input_and_long_regions(ctx):
    """Check 2: all of check 1 again with every tile on the generic path (test option region_assemble_generic), then, unforced,
    regions that a tile cannot take: one region of 3 000 rows, 46 regions of 12 rows, a region that starts on the last row of what
    would be a full tile — each between ordinary regions, so both paths run in one launch."""
    ctx.set_option("region_assemble_generic", 1)
    try:
        assert run_shapes(ctx)
    finally:
        ctx.set_option("region_assemble_generic", 0)
    sh = Shapes(ctx, 8)
    rng = np.random.default_rng(99)
    ordinary = lambda k: list(rng.integers(1, 12, k))
    full_tile = [11] * 41 + [15] * 4                                  # 45 regions, 511 rows: the 46th starts on row 511
    assert sum(full_tile) == 511 and len(full_tile) == 45
    for tag, spans in (("one region of 3000 rows", ordinary(46 * 3) + [3000] + ordinary(200)),
                       ("46 regions of 12 rows", ordinary(46 * 2) + [12] * 46 + ordinary(200)),
                       ("a region from the last row of a full tile", ordinary(46) + full_tile + [11] + ordinary(300)),
                       ("long regions only", [700, 0, 513, 1, 2000])):
        ptr = np.concatenate([[0], np.cumsum(spans)]).astype(np.int64)
        assert ptr[-1] <= len(sh.rb)
        for off in (0, 1):
            sh.check(int(ptr[-1]) + off, off, ptr=ptr, tag=tag)
    with pytest.raises(Exception):
        ctx.set_option("region_assemble_generic", 2)


@gpu
def test_binding_refuses_bad_arguments_before_any_launch(ctx):
    """Check 3: wrong dtype, a CPU tensor, a non-contiguous view, len(keys) != len(vals), S = 65, a distfun of the wrong shape ->
    ValueError, and the C entry point is never reached."""
    import torch
    from assemble_inputs import assemble
    sh = Shapes(ctx, 3)
    db, do = sh.db[:100], sh.do[:100]
    ptr = sh.t(np.array([0, 40, 100], dtype=np.int64))
    bg = list(sh.bg)

    class NoLaunch:
        def __init__(self, lib):
            self._lib = lib

        def __getattr__(self, name):
            if name == "chicdiff_hip_region_assemble_dev":
                raise AssertionError("the entry point was reached")
            return getattr(self._lib, name)

    lib = ctx.lib
    ctx.lib = NoLaunch(lib)
    try:
        bad_sj = torch.zeros((sh.S, 2 * bg[2].shape[1]), dtype=torch.float64, device=ctx.device)[:, ::2]
        assert bad_sj.shape == bg[2].shape and not bad_sj.is_contiguous()
        k0, v0 = sh.tabs[0]
        for tag, args in (
                ("dtype of bait", (db.to(torch.int64), do, ptr, sh.tabs, bg)),
                ("dtype of region_ptr", (db, do, ptr.to(torch.int32), sh.tabs, bg)),
                ("dtype of vals", (db, do, ptr, [(k0, v0.to(torch.int64))] + sh.tabs[1:], bg)),
                ("dtype of si", (db, do, ptr, sh.tabs, bg[:3] + [bg[3].to(torch.float32)] + bg[4:])),
                ("CPU tensor", (db.cpu(), do, ptr, sh.tabs, bg)),
                ("CPU table", (db, do, ptr, [(k0.cpu(), v0.cpu())] + sh.tabs[1:], bg)),
                ("non-contiguous", (db, do, ptr, sh.tabs, bg[:2] + [bad_sj] + bg[3:])),
                ("non-contiguous rows", (sh.db[:200:2], do, ptr, sh.tabs, bg)),
                ("keys != vals", (db, do, ptr, [(k0, v0[:-1])] + sh.tabs[1:], bg)),
                ("S = 65", (db, do, ptr, sh.tabs * 22, bg)),          # 66 tables
                ("S = 0", (db, do, ptr, [], bg)),
                ("distfun shape", (db, do, ptr, sh.tabs, bg[:7] + [bg[7][:, :9]])),
                ("oe shorter than bait", (db, do[:-1], ptr, sh.tabs, bg))):
            with pytest.raises(ValueError):
                assemble(ctx, args[0], args[1], args[2], args[3], tuple(args[4]))
                pytest.fail(tag)
        assert len(sh.tabs * 22) == 66 and len((sh.tabs * 22)[:65]) == 65
        with pytest.raises(ValueError, match="64"):
            assemble(ctx, db, do, ptr, (sh.tabs * 22)[:65], tuple(bg))
        with pytest.raises(AssertionError, match="entry point was reached"):   # the guard itself: a good call does reach it
            assemble(ctx, db, do, ptr, sh.tabs, tuple(bg))
    finally:
        ctx.lib = lib
    assemble(ctx, db, do, ptr, sh.tabs, tuple(bg))


@gpu
def test_pipeline_assemble_gives_the_same_result_tables(ctx, tmp_path):
    """Check 4: getFullRegionData(assemble=True) -> DESeq2Wrap against the default path, every column bit for bit, for the test and
    the control block and the three norm modes."""
    from chicdiff_amd import pipeline
    from pipeline_inputs import make_experiment, read_chicago_pickle
    settings, _ = make_experiment(tmp_path, npeaks=2500, with_chinput=True)
    RU = pipeline.getRegionUniverse(settings, ctx)
    RUc = pipeline.getControlRegionUniverse(settings, RU, ctx, rng=np.random.default_rng(11))
    frd = pipeline.getFullRegionData(settings, RU, RUc, ctx=ctx, read_chicago=read_chicago_pickle)
    frd_a = pipeline.getFullRegionData(settings, RU, RUc, ctx=ctx, read_chicago=read_chicago_pickle, assemble=True)
    for blk, blk_a in zip(frd[:2], frd_a[:2]):
        assert "fragN" in blk and "fragN" not in blk_a and "fragFullMean" not in blk_a
        S, n = blk["S"], blk["n"]
        assert blk_a["regionN"].shape == (S, n) and blk_a["regionFullMean"].shape == (S, n)
        assert_same((blk_a["regionN"], blk_a["regionFullMean"]), ctx.window_sums(blk["fragN"], blk["fragFullMean"], blk["region_ptr"]), "block")
        assert blk_a["region_ptr"] is blk["region_ptr"] or (blk_a["region_ptr"] == blk["region_ptr"]).all()
        assert (blk_a["avDist"] == blk["avDist"]).all() and blk_a["is_control"] == blk["is_control"]
    for norm in ("standard", "fullmean", "combined"):
        st = dict(settings, norm=norm)
        theta = None
        for u, blk, blk_a, suffix in ((RU, frd[0], frd_a[0], ""), (RUc, frd[1], frd_a[1], "Control")):
            ref = pipeline.DESeq2Wrap(st, u, blk, suffix=suffix, theta=theta, ctx=ctx)
            got = pipeline.DESeq2Wrap(st, u, blk_a, suffix=suffix, theta=theta, ctx=ctx)
            assert list(got.columns) == list(ref.columns) and len(got) == len(ref) == blk["n"] and got.attrs == ref.attrs
            for col in ref.columns:
                a, b = got[col].to_numpy(), ref[col].to_numpy()
                if a.dtype == np.float64:
                    nan = np.isnan(b)
                    assert np.array_equal(np.isnan(a), nan) and np.array_equal(a.view(np.int64)[~nan], b.view(np.int64)[~nan]), (norm, suffix, col)
                else:
                    assert a.dtype == b.dtype and np.array_equal(a, b), (norm, suffix, col)
            assert np.isfinite(ref["pvalue"].to_numpy()).any()
            theta = ref.attrs.get("theta")                            # the control fit inherits the test fit's theta (chicdiff.R:331-332)


def searchsorted_total(torch, rukey, tables):
    """Sum of the values of the keys the RU rows hit, per table, by torch.searchsorted: independent of the library's joins."""
    out = []
    for ks, vs in tables:
        if ks.numel() == 0:
            out.append(0)
            continue
        at = torch.searchsorted(ks, rukey).clamp(max=ks.numel() - 1)
        hit = ks[at] == rukey
        out.append(int(vs[at][hit].to(torch.int64).sum()))
    return out


@gpu
def test_end_to_end_size_2M_x8(ctx):
    """Check 5: the benchmark's end-to-end shape (2 M peaks x 8 replicates, RUexpand = 5, inputs by tests/assemble_inputs.py):
    equal to the three calls, and the integer identity sum(N) = sum of the joined counts."""
    import torch
    from assemble_inputs import assemble, background_args, make, three_calls
    d = make(ctx, 2_000_000, 8, counts="synth")
    bg = background_args(d)
    assert d["nfrag"] > 10 * d["n"] and int((d["region_ptr"][1:] - d["region_ptr"][:-1]).max()) <= 11
    N, FM = assemble(ctx, d["bait"], d["oe"], d["region_ptr"], d["tables"], bg)
    Nr, FMr = three_calls(ctx, d["bait"], d["oe"], d["region_ptr"], d["tables"], bg)
    assert torch.equal(N, Nr)
    assert_same((N, FM), (Nr, FMr), "2 M x 8")
    if not torch.isnan(FMr).any():
        assert torch.equal(FM, FMr)
    joined = ctx.count_join_multi(d["bait"], d["oe"], d["tables"]).to(torch.int64).sum(1)
    assert torch.equal(N.to(torch.int64).sum(1), joined) and int(joined.min()) > 0
    rukey = d["bait"].to(torch.int64) * (1 << 32) + d["oe"].to(torch.int64)
    assert N.to(torch.int64).sum(1).tolist() == searchsorted_total(torch, rukey, d["tables"])


@gpu
def test_full_size_20M_x16_upstream_half(ctx):
    """Check 6: region universe -> region_assemble at BASELINE's largest configuration, 20 M peaks x 16 replicates (inputs on the
    device from a seed, every table a quarter of the pairs).  Bit for bit against the three calls on a contiguous slice of 200 000
    regions (on the slice's rows only: the two 41 GB matrices never exist), and sum(N) over ALL regions against the values of the
    keys hit, by torch.searchsorted per table."""
    import torch
    from assemble_inputs import assemble, background_args, make, three_calls
    n, S = 20_000_000, 16
    d = make(ctx, n, S, counts="device", table_share=0.25)
    bg = background_args(d)
    assert d["nfrag"] > 10 * n
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    before = torch.cuda.memory_allocated()
    N, FM = assemble(ctx, d["bait"], d["oe"], d["region_ptr"], d["tables"], bg)
    assert N.shape == (S, n) and FM.shape == (S, n)
    assert torch.cuda.max_memory_allocated() - before <= 12 * S * n + (64 << 20)     # the outputs, nothing of size S x nfrag
    i0 = 7_654_321
    i1 = i0 + 200_000
    ptr = d["region_ptr"]
    f0, f1 = int(ptr[i0]), int(ptr[i1])
    ref = three_calls(ctx, d["bait"][f0:f1], d["oe"][f0:f1], (ptr[i0:i1 + 1] - f0).contiguous(), d["tables"], bg)
    assert_same((N[:, i0:i1].contiguous(), FM[:, i0:i1].contiguous()), ref, "slice")
    assert bool((ref[0] > 0).any())
    rukey = d["bait"].to(torch.int64) * (1 << 32) + d["oe"].to(torch.int64)
    total = searchsorted_total(torch, rukey, d["tables"])
    assert N.to(torch.int64).sum(1).tolist() == total and min(total) > 0
