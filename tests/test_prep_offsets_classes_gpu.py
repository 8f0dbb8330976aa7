"""prep16_kernel / offsets16_kernel by sample class (register arrays of 4, 8 or 16 samples) with the next tile's loads in flight:
the offsets formed inside prep (option fuse_offsets = 2) against the launch of their own (0), bit for bit, at the class edges
(S = 4 | 5, 8 | 9, 16 | 17 and the switch from 256- to 128-row tiles above S = 8), at row counts of one row, one row short of and one
row past a 256-row tile, and at 2051 rows on four workgroups (option prep_blocks), where a workgroup walks several tiles — one of them
three, its last tile of 3 rows, the others two (S <= 8; five and four 128-row tiles above).  Planted: all-zero rows first, last and
(2051 rows) filling the whole second tile; NA in FullMean in row 0, in the last row and in the first row of the partial tile."""
import functools

import numpy as np
import pytest

from chicdiff_amd import synth

pytestmark = pytest.mark.gpu

SHAPES_S = (2, 3, 4, 5, 8, 9, 12, 16)
ROWS = ((1, 0), (255, 0), (257, 0), (2051, 4))  # (rows, prep_blocks)
THETAS = (0.0, 0.5, 1.0, None)                  # None: no mixing


@pytest.fixture(scope="module")
def ctx():
    import __graft_entry__ as g
    g.build()  # no-op when the in-tree library and the oracle are up to date
    from chicdiff_amd import hip
    c = hip.HipContext(0)
    yield c
    c.set_option("fuse_offsets", 1)
    c.set_option("prep_blocks", 0)
    c.close()


@pytest.fixture(scope="module")
def oracle():
    from oracle import oracle as o
    return o


def tile_rows(S):
    return 256 if S <= 8 else 128  # a row record of more than 128 bytes (S > 8): 128-row tiles


@functools.lru_cache(maxsize=None)
def base_inputs(S):
    d = synth.make(2051, S)
    return d["counts"], d["nf"] * (d["mu"][:, None] / S)


def group_of(S):
    return np.zeros(2, dtype=np.int32) if S == 2 else synth.groups(S)  # (two samples leave a two-level design no residual d.f.)


def planted(S, n):
    """The first n rows of the synthetic matrix with the rows the tile logic can get wrong: (counts, FullMean), both (n, S)."""
    counts, fm = (a[:n].copy() for a in base_inputs(S))
    T = tile_rows(S)
    if n == 1:
        counts[0] = np.maximum(counts[0], 1)  # the one row has to carry the size factors
        return counts, fm
    counts[0] = 0
    counts[n - 1] = 0
    if n >= 3 * T:
        counts[T:2 * T] = 0
    fm[0, 0] = np.nan
    fm[n - 1, S - 1] = np.nan
    partial = (n // T) * T  # first row of the partial last tile
    if n % T:
        fm[partial, 1 % S] = np.nan
    return counts, fm


def run(ctx, dk, dfm, group, theta, fuse, blocks, want=None):
    """One wald_test through one route: ({column: array}, scalars), or the error it raised as a string."""
    from chicdiff_amd import hip
    ctx.set_option("fuse_offsets", fuse)
    ctx.set_option("prep_blocks", blocks)
    try:
        out, sc = ctx.wald_test(dk, dfm, group, theta=theta, want=want if want is not None else hip.OUT_DOUBLE + hip.OUT_INT)
    except hip.ChicdiffHipError as e:
        return str(e)
    finally:
        ctx.set_option("fuse_offsets", 1)
        ctx.set_option("prep_blocks", 0)
    return {k: v.cpu().numpy() for k, v in out.items()}, sc


def same(a, b):
    a, b = np.asarray(a), np.asarray(b)
    return np.array_equal(a, b, equal_nan=a.dtype.kind == "f")


def assert_same_results(a, b, tag):
    assert isinstance(a, str) == isinstance(b, str), (tag, a if isinstance(a, str) else "ok", b if isinstance(b, str) else "ok")
    if isinstance(a, str):
        assert a == b, tag
        return
    (oa, sa), (ob, sb) = a, b
    assert set(oa) == set(ob) and set(sa) == set(sb)
    for k in oa:
        assert same(oa[k], ob[k]), f"{tag} {k}: {int(np.sum(~((oa[k] == ob[k]) | ((oa[k] != oa[k]) & (ob[k] != ob[k])))))} rows differ"
    for k in sa:
        assert same(sa[k], sb[k]), (tag, k, sa[k], sb[k])


@pytest.mark.parametrize("S", SHAPES_S)
def test_offsets_inside_prep_equal_their_own_launch(ctx, S):
    """Every output column wald_test offers and every returned scalar, offsets inside prep against a launch of their own at the same
    prep_blocks; theta 0, 0.5, 1 and no mixing.  A fit the library refuses (one row carries no trend) has to be refused alike."""
    group = group_of(S)
    fits = 0
    for n, blocks in ROWS:
        counts, fm = planted(S, n)
        dk, dfm = ctx.to_device(counts, np.int32), ctx.to_device(fm, np.float64)
        for theta in THETAS:
            a = run(ctx, dk, dfm, group, theta, 0, blocks)
            b = run(ctx, dk, dfm, group, theta, 2, blocks)
            assert_same_results(a, b, f"S={S} n={n} theta={theta}")
            if not isinstance(a, str):
                fits += 1
                if n > 1:  # the planted rows are what they were planted as
                    assert a[0]["allZero"][0] == 1 and a[0]["allZero"][n - 1] == 1 and a[1]["nAllZero"] >= (2 + tile_rows(S) if blocks else 2)
    assert fits >= 3 * len(THETAS), "the fits of 255, 257 and 2051 rows must go through"


def test_prep_blocks_does_not_change_the_results(ctx):
    """Four workgroups that walk several tiles each give what one resident round of single tiles gives (the block sums of the nf
    columns are double-double: the same rounded sum in any grouping)."""
    counts, fm = planted(8, 2051)
    dk, dfm = ctx.to_device(counts, np.int32), ctx.to_device(fm, np.float64)
    for fuse in (0, 2):
        assert_same_results(run(ctx, dk, dfm, group_of(8), 0.5, fuse, 0), run(ctx, dk, dfm, group_of(8), 0.5, fuse, 4), f"fuse_offsets={fuse}")


def test_theta_grid_deviances_both_routes(ctx):
    """The grid's deviance totals (sum() without na.rm: an all-zero row makes a total NA, so those rows are left out here — the NA
    rows of FullMean stay), four workgroups over seven tiles."""
    counts, fm = planted(8, 2051)
    keep = counts.sum(1) > 0
    counts, fm = counts[keep], fm[keep]
    assert len(counts) > 6 * 256 and np.isnan(fm).any()
    dk, dfm = ctx.to_device(counts, np.int32), ctx.to_device(fm, np.float64)
    sf = ctx.size_factors(dk)
    thetas = [0.0, 0.25, 0.5, 0.75, 1.0]
    dev = {}
    try:
        ctx.set_option("prep_blocks", 4)
        for fuse in (0, 2):
            ctx.set_option("fuse_offsets", fuse)
            dev[fuse] = ctx.theta_grid(dk, dfm, sf, thetas)
    finally:
        ctx.set_option("fuse_offsets", 1)
        ctx.set_option("prep_blocks", 0)
    assert np.all(np.isfinite(dev[0])) and len(set(dev[0])) == len(thetas)
    assert np.array_equal(dev[0], dev[2]), (dev[0], dev[2])


@pytest.mark.parametrize("S", (4, 8, 16))
def test_negative_count_in_the_partial_tile_is_refused(ctx, S):
    """A negative count (NA_integer_) in the 3-row last tile of 2051 rows: refused with the same status through both routes."""
    counts, fm = planted(S, 2051)
    counts[2049, S - 1] = -2147483648
    dk, dfm = ctx.to_device(counts, np.int32), ctx.to_device(fm, np.float64)
    a = run(ctx, dk, dfm, group_of(S), 0.5, 0, 4, want=["pvalue"])
    b = run(ctx, dk, dfm, group_of(S), 0.5, 2, 4, want=["pvalue"])
    assert isinstance(a, str) and "counts contain a negative value or NA_integer_" in a, a
    assert a == b


@pytest.mark.parametrize("S", (3, 4, 5, 9, 16))
def test_offsets_kernel_by_class_against_oracle(ctx, oracle, S):
    """ctx.offsets (offsets16_kernel, by class) against the oracle at the tolerance test_offsets_and_window_sums uses."""
    for n in (1, 257):
        _, fm = planted(S, n)
        sf = np.exp(np.linspace(-0.3, 0.3, S))
        dfm = ctx.to_device(fm, np.float64)
        for theta in (None, 0.0, 0.25, 1.0):
            got = ctx.offsets(dfm, sf, theta).cpu().numpy().T
            ref = oracle.offsets(fm, sf, theta)
            assert not np.isnan(ref).any() and np.allclose(got, ref, rtol=1e-13), (S, n, theta)


def test_17_samples_take_the_general_kernels(ctx, oracle):
    """S = 17 is past the classes: the offsets stay a launch of their own whatever fuse_offsets says (the "offsets" timing scope is
    there), through the general kernel, and the fit through the general prep — same results either way."""
    S = 17
    counts, fm = planted(S, 257)
    dk, dfm = ctx.to_device(counts, np.int32), ctx.to_device(fm, np.float64)
    sf = np.exp(np.linspace(-0.3, 0.3, S))
    assert np.allclose(ctx.offsets(dfm, sf, 0.25).cpu().numpy().T, oracle.offsets(fm, sf, 0.25), rtol=1e-13)
    try:
        ctx.enable_timing(1)
        b = run(ctx, dk, dfm, group_of(S), 0.5, 2, 4)
        scopes = ctx.kernel_times()
    finally:
        ctx.enable_timing(0)
    assert scopes["offsets"][1] == 1 and scopes["prep"][1] == 1
    assert_same_results(run(ctx, dk, dfm, group_of(S), 0.5, 0, 0), b, "S=17")
