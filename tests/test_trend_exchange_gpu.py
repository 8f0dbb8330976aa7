"""The persistent trend kernel's exchange of partial sums as self-tagged words (option "trend_exchange", chicdiff_amd/csrc/
trend_kernels.hip): the passes after the first cross no grid barrier, every workgroup polls the others' words instead.  The sums
are added in the order of the barrier route, so no bit may change: every case is fitted with "trend_exchange" 0 (publish, grid
barrier, re-read) and 1, and every per-row output, the trend coefficients, varLogDispEsts, dispPriorVar, trendOuterIter, status and
sumDeviance must be identical.  After every fit the context must report no refit and a trend that did not fail: a kernel that gave
up on its exchange would send the fit to the one-launch-per-pass route, and the comparison would compare nothing.
(The words and the protocol themselves are checked on the CPU: tests/test_trend_exchange.py.)"""
import numpy as np
import pytest

from chicdiff_amd import synth

pytestmark = pytest.mark.gpu

TRENDFAILED, TREND_LOCAL = 1, 16
SCALARS = ("trendCoef", "varLogDispEsts", "dispPriorVar", "trendOuterIter", "status", "sumDeviance")


@pytest.fixture(scope="module")
def ctx():
    import __graft_entry__ as g
    g.build()  # no-op when the in-tree library and the oracle are up to date
    from chicdiff_amd import hip
    c = hip.HipContext(0)
    yield c
    c.close()


_data = {}


def data(n, S):
    """(device counts, device nf, group) of synth.make(n, S): made once per shape, never changed"""
    if (n, S) not in _data:
        _data[(n, S)] = synth.make(n, S)
    return _data[(n, S)]


def fit(ctx, d, dev, exchange, want):
    """one fit by the given exchange route: it must have come from the persistent kernel, at the first attempt"""
    ctx.set_option("trend_exchange", exchange)
    out, sc = ctx.nbglm_fit(dev[0], dev[1], d["group"], want=want)
    assert ctx.last_refits() == 0, ("refits", exchange, ctx.last_refits())
    assert (sc["status"] & (TRENDFAILED | TREND_LOCAL)) == 0, ("status", exchange, sc["status"])
    return {k: out[k].cpu().numpy().copy() for k in want}, sc


def same(a, b, what):
    (out_a, sc_a), (out_b, sc_b) = a, b
    for k in SCALARS:
        assert np.asarray(sc_a[k], np.float64).tobytes() == np.asarray(sc_b[k], np.float64).tobytes(), (what, k, sc_a[k], sc_b[k])
    for k in out_a:
        assert out_a[k].tobytes() == out_b[k].tobytes(), (what, k, int(np.sum(out_a[k] != out_b[k])))


CASES = {
    # name: (rows, samples, options besides the one under test)
    "one_workgroup_1500x4": (1500, 4, {}),
    "two_workgroups_2051x4": (2051, 4, {}),                    # the smallest exchange
    "65_workgroups_131073x4": (131073, 4, {}),                 # lane 0's second stride alone
    "256_workgroups_522241x4": (522241, 4, {}),
    "rows_beyond_the_lds_cache_70000x8": (70000, 8, {"trend_persistent_blocks": 2}),  # 35 000 rows per workgroup, 8 000 cached
}


@pytest.mark.parametrize("speculate", [0, 1])  # 8-word and 16-word slots
@pytest.mark.parametrize("name", list(CASES))
def test_same_bits_as_the_barrier_route(ctx, name, speculate):
    from chicdiff_amd import hip
    n, S, extra = CASES[name]
    d = data(n, S)
    dev = (ctx.to_device(d["counts"], np.int32), ctx.to_device(d["nf"], np.float64))
    want = hip.OUT_DOUBLE + hip.OUT_INT
    try:
        for k, v in extra.items():
            ctx.set_option(k, v)
        ctx.set_option("trend_speculate", speculate)
        ref = fit(ctx, d, dev, 0, want)
        got = fit(ctx, d, dev, 1, want)
    finally:
        ctx.set_option("trend_exchange", 1)
        ctx.set_option("trend_speculate", 1)
        for k in extra:
            ctx.set_option(k, 0)
    print(name, speculate, ref[1])
    assert np.isfinite(ref[1]["varLogDispEsts"]) and ref[1]["trendOuterIter"] >= 1
    same(got, ref, name)


def test_radix_selects_behind_unfenced_passes(ctx):
    """"mad_select_route" = 0: six real grid barriers follow the passes that crossed none — their counters must have counted the
    real ones alone"""
    from chicdiff_amd import hip
    d = data(30000, 8)
    dev = (ctx.to_device(d["counts"], np.int32), ctx.to_device(d["nf"], np.float64))
    want = hip.OUT_DOUBLE + hip.OUT_INT
    try:
        ctx.set_option("mad_select_route", 0)
        ref = fit(ctx, d, dev, 0, want)
        got = fit(ctx, d, dev, 1, want)
    finally:
        ctx.set_option("trend_exchange", 1)
        ctx.set_option("mad_select_route", 1)
    same(got, ref, "radix")


def test_fits_in_a_row_on_one_context(ctx):
    """a larger grid, a smaller one, the larger one again, all in one workspace: every fit starts from cleared words, and a grid of
    two workgroups never looks at what fifteen left behind"""
    from chicdiff_amd import hip
    want = hip.OUT_DOUBLE + hip.OUT_INT
    shapes = [(30000, 8), (2051, 4), (30000, 8)]
    dev = {s: (ctx.to_device(data(*s)["counts"], np.int32), ctx.to_device(data(*s)["nf"], np.float64)) for s in set(shapes)}
    try:
        ref = {s: fit(ctx, data(*s), dev[s], 0, want) for s in set(shapes)}
        got = [fit(ctx, data(*s), dev[s], 1, want) for s in shapes]
    finally:
        ctx.set_option("trend_exchange", 1)
    for s, g in zip(shapes, got):
        same(g, ref[s], s)


def test_twelve_fits_give_one_answer(ctx):
    """250 000 x 8, where an exchange whose validity travelled apart from the data was once seen to vary from run to run: a
    comparison of results"""
    d = data(250000, 8)
    dev = (ctx.to_device(d["counts"], np.int32), ctx.to_device(d["nf"], np.float64))
    want = ["dispersion"]
    try:
        runs = [fit(ctx, d, dev, 1, want) for _ in range(12)]
    finally:
        ctx.set_option("trend_exchange", 1)
    for out, sc in runs[1:]:
        for k in ("trendCoef", "varLogDispEsts"):
            assert np.asarray(sc[k], np.float64).tobytes() == np.asarray(runs[0][1][k], np.float64).tobytes(), (k, sc[k], runs[0][1][k])
        assert out["dispersion"].tobytes() == runs[0][0]["dispersion"].tobytes()
