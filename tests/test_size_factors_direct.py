"""Size factors of a single-rank call in two passes over the counts (chicdiff_amd/csrc/global_kernels.hip: "size factors in two passes
over the counts"; common.h: sf_bin, sf_sub_bin).

The medians of log(count) - row log geometric mean are exact order statistics whichever way they are found, so the direct route — value
bins, pick, lists of the picked bins' keys, finish — must give the size factors of the radix select over stored keys (option
"select_all_rounds" = 1) bit for bit.  Its exactness rests on the bin functions never decreasing as the key grows; they are plain
functions compiled for the host too (chicdiff_hip_selftest_sf_bin).  CPU part: that property, and a numpy restatement of histogram ->
pick -> list -> order statistic on the library's own bins against np.sort.  GPU part: both routes and the oracle on the same inputs."""
import ctypes as C
import time

import numpy as np
import pytest

from chicdiff_amd import synth

CAND = 1024  # kSfCand: keys of one sub-bin ranked by counting
SUB_BINS = 4096
LO, SPAN = -4.0, 8.0


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as g
    g.build()
    from chicdiff_amd import hip
    return hip.load_library()


def lib_bins(L, S, x, sub_of=None):
    """(bins per column, bin of each x, sub-bin of each x inside bin `sub_of`) by the library's functions"""
    x = np.ascontiguousarray(x, dtype=np.float64)
    b = np.zeros(len(x), dtype=np.int32)
    sb = np.zeros(len(x), dtype=np.int32)
    ip, dp = C.POINTER(C.c_int32), C.POINTER(C.c_double)
    nb = C.c_int32(0)
    rc = L.chicdiff_hip_selftest_sf_bin(S, x.ctypes.data_as(dp), len(x), C.byref(nb), b.ctypes.data_as(ip), 0 if sub_of is None else int(sub_of),
                                        None if sub_of is None else sb.ctypes.data_as(ip))
    assert rc == 0
    return int(nb.value), b, sb


# ---- inputs --------------------------------------------------------------------------------------------------------------------------

def tie_cases():
    rng = np.random.default_rng(5)  # tests/test_gpu_parity.py::test_size_factors_with_massive_ties, both of its matrices
    n, S = 60000, 4
    counts = rng.poisson(30, size=(n, S)).astype(np.int32)
    counts[: 2 * n // 3] = [10, 20, 30, 41]
    counts = counts[rng.permutation(n)]
    counts2 = np.concatenate([np.tile(np.array([[8, 16, 24, 33]], np.int32), (9000, 1)), np.tile(np.array([[9, 15, 25, 30]], np.int32), (9000, 1))])
    return counts, counts2


def split_middles():
    """S = 2, an even number of used rows, half of them with count ratios near e^-2 and half near e^2: column 0's keys are +-1, so its two
    middle order statistics lie a thousand bins apart (column 1 mirrors it)"""
    rng = np.random.default_rng(77)
    a = rng.integers(50, 150, 5000)
    b = np.rint(a * np.exp(2.0) * rng.uniform(0.9, 1.1, 5000)).astype(np.int64)
    rows = np.concatenate([np.stack([a[:2500], b[:2500]], 1), np.stack([b[2500:], a[2500:]], 1)]).astype(np.int32)
    return np.ascontiguousarray(rows[rng.permutation(5000)])


def zeros_and_negatives():
    rng = np.random.default_rng(11)
    k = rng.poisson(3.0, size=(40000, 6)).astype(np.int32)  # plenty of zero counts
    k[rng.integers(0, 40000, 500), rng.integers(0, 6, 500)] = -1
    k[rng.integers(0, 40000, 50), rng.integers(0, 6, 50)] = np.iinfo(np.int32).min  # NA_integer_
    return k


def scaled(factor):
    rng = np.random.default_rng(13)
    k = (rng.poisson(50.0, size=(20000, 4)) + 1).astype(np.int64)
    k[:, 2] *= factor
    assert k.max() < 2 ** 31
    return k.astype(np.int32)


def cases(full):
    """name -> counts (n x S).  full: with the shapes that are too slow for the numpy restatement"""
    c = {}
    for n, S in [(7, 3), (1001, 4), (100, 8), (50_000, 8), (300_000, 16)] + ([(2_000_000, 8)] if full else []):
        c[f"synth_{n}x{S}"] = synth.make(n, S)["counts"]
    rng = np.random.default_rng(3)
    col = rng.poisson(40.0, 3001).astype(np.int32) + 1
    c["equal_columns"] = np.stack([col, col], 1)  # every ratio is exactly 0
    c["massive_ties"], c["two_tied_values"] = tie_cases()
    c["split_middles"] = split_middles()
    c["zeros_and_negatives"] = zeros_and_negatives()
    c["column_x1000"] = scaled(1000)        # that column's keys: + 5.2, beyond the last bin; the others': - 1.7
    c["column_x1000000"] = scaled(1000000)  # + 10.4 and - 3.5
    return c


def keys_of(counts):
    """the select's keys in numpy: column j of the used rows (every count > 0)"""
    k = np.asarray(counts, dtype=np.float64)
    with np.errstate(divide="ignore", invalid="ignore"):
        l = np.log(k)
    lg = l.sum(1) / k.shape[1]
    use = np.isfinite(lg)
    return (l[use] - lg[use, None])


# ---- CPU: the bin functions --------------------------------------------------------------------------------------------------------------

def sorted_probe():
    rng = np.random.default_rng(1)
    tiny = np.array([0.0, 5e-324, 2.2250738585072014e-308, 1e-300, 1e-20])
    big = np.array([21.4875626, 31 * np.log(2.0), 1e3, 1e300, np.finfo(np.float64).max])  # log(2^31 - 1) is the largest key there is
    edges = LO + SPAN * np.arange(0, 3841) / 3840.0
    x = np.concatenate([-big, -tiny, tiny, big, [LO, LO + SPAN, np.nextafter(LO, -1), np.nextafter(LO, 1), np.nextafter(LO + SPAN, -1e9),
                                                np.nextafter(LO + SPAN, 1e9)],
                        edges, np.nextafter(edges, -1e9), np.nextafter(edges, 1e9), rng.uniform(-5, 5, 200000), rng.normal(0, 0.3, 200000)])
    x = np.sort(x)
    k = int(np.searchsorted(x, 0.0))
    return np.concatenate([x[:k], [-0.0], x[k:]])  # -0 in front of +0, as the select's key order has them


@pytest.mark.parametrize("S", [1, 2, 4, 5, 8, 9, 16])
def test_bin_functions_never_decrease(lib, S):
    x = sorted_probe()
    nb, b, _ = lib_bins(lib, S, x)
    assert nb == 15360 // (4 if S <= 4 else 8 if S <= 8 else 16)
    assert b.min() == 0 and b.max() == nb - 1
    assert np.all(np.diff(b) >= 0)
    # restated: clamp(floor((x - lo) * (nb / span)), 0, nb - 1)
    with np.errstate(over="ignore"):
        want = np.clip(np.floor((x - LO) * (nb / SPAN)), 0, nb - 1).astype(np.int32)
    assert np.array_equal(b, want)
    assert b[np.flatnonzero(x == 0.0)].min() == b[np.flatnonzero(x == 0.0)].max() == nb // 2  # -0, +0
    for of in (0, 1, nb // 2 - 1, nb // 2, nb - 2, nb - 1):
        _, _, sb = lib_bins(lib, S, x, sub_of=of)
        assert sb.min() == 0 and sb.max() == SUB_BINS - 1
        assert np.all(np.diff(sb) >= 0), of
        inside = np.flatnonzero(b == of)
        if 0 < of < nb - 1:  # an inner bin's keys spread over its sub-bins; everything below / above it sits in the first / last one
            assert np.all(sb[: inside[0]] == 0) and np.all(sb[inside[-1] + 1:] == SUB_BINS - 1)
            assert len(np.unique(sb[inside])) > 1


def test_bins_reject_bad_arguments(lib):
    x = np.zeros(1)
    b = np.zeros(1, dtype=np.int32)
    ip, dp = C.POINTER(C.c_int32), C.POINTER(C.c_double)
    for S in (0, 17, -1):
        assert lib.chicdiff_hip_selftest_sf_bin(S, x.ctypes.data_as(dp), 1, None, b.ctypes.data_as(ip), 0, None) == 1  # CHICDIFF_E_INVALID


# ---- CPU: histogram -> pick -> list -> order statistic, restated -----------------------------------------------------------------------

def pick(hist, rank):
    """fit_state.h sel_pick: the first bin whose running total exceeds the rank, else the last; and the rank inside it"""
    cum = np.cumsum(hist)
    b = int(np.searchsorted(cum, rank, side="right"))
    b = min(b, len(hist) - 1)
    return b, int(rank - (cum[b] - hist[b]))


def direct_medians(L, counts):
    """the two middle order statistics of every column by the direct select's steps, on the library's bins; and what it met on the way"""
    keys = keys_of(counts)
    m, S = keys.shape
    out = np.full((S, 2), np.nan)
    seen = dict(split=0, fallback=0, longest_list=0)
    if m == 0:
        return out, seen
    for j in range(S):
        x = keys[:, j]
        nb, b, _ = lib_bins(L, S, x)
        hist = np.bincount(b, minlength=nb)                      # pass 1
        assert hist.sum() == m
        picks = [pick(hist, (m - 1) // 2), pick(hist, m // 2)]   # pick
        seen["split"] += picks[0][0] != picks[1][0]
        for slot, (pb, rin) in enumerate(picks):
            lst = x[b == pb]                                      # pass 2 (in any order: shuffle it)
            lst = lst[np.random.default_rng(j).permutation(len(lst))]
            seen["longest_list"] = max(seen["longest_list"], len(lst))
            _, _, sb = lib_bins(L, S, lst, sub_of=pb)             # finish
            sh = np.bincount(sb, minlength=SUB_BINS)
            psb, r2 = pick(sh, rin)
            cand = lst[sb == psb]
            if len(cand) <= CAND:
                less = np.array([(cand < v).sum() + (cand[:t] == v).sum() for t, v in enumerate(cand)])  # ranked by counting
                out[j, slot] = cand[np.flatnonzero(less == r2)[0]]
            else:  # massive ties, keys beyond the binned range: an exact select over the whole list
                seen["fallback"] += 1
                out[j, slot] = np.sort(lst)[rin]
    return out, seen


def test_restated_select_equals_sorting(lib):
    met = dict(split=0, fallback=0, longest_list=0)
    for name, counts in cases(full=False).items():
        got, seen = direct_medians(lib, counts)
        keys = np.sort(keys_of(counts), axis=0)
        m = keys.shape[0]
        assert m > 0, name
        want = np.stack([keys[(m - 1) // 2], keys[m // 2]], 1)
        assert np.array_equal(got, want), name
        print(name, "used rows", m, seen)
        for k in met:
            met[k] = max(met[k], seen[k])
        if name == "split_middles":
            assert seen["split"] == 2
        if name in ("massive_ties", "two_tied_values", "column_x1000", "column_x1000000"):
            assert seen["fallback"] > 0, name
    assert met["split"] and met["fallback"] and met["longest_list"] > CAND


# ---- GPU: both routes and the oracle ------------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def ctxs():
    import __graft_entry__ as g
    g.build()
    from chicdiff_amd import hip
    direct, classic = hip.HipContext(0), hip.HipContext(0)
    classic.set_option("select_all_rounds", 1)
    yield direct, classic
    direct.close()
    classic.close()


@pytest.mark.gpu
def test_direct_route_equals_radix_select_and_oracle(ctxs):
    from oracle import oracle
    direct, classic = ctxs
    for name, counts in cases(full=True).items():
        dk = direct.to_device(counts, np.int32)
        got = direct.size_factors(dk)
        ref = classic.size_factors(dk)
        again = direct.size_factors(dk)  # the histograms were left zero
        orc = oracle.size_factors(counts)
        err = np.max(np.abs(got - orc) / np.abs(orc))
        print(f"{name}: {counts.shape[0]} x {counts.shape[1]} size factors {got} max rel. distance from the oracle {err:.2e}")
        assert np.all(np.isfinite(ref)), name
        assert np.array_equal(got, ref), (name, got, ref)
        assert np.array_equal(again, got), name
        assert np.allclose(got, orc, rtol=1e-13), (name, got, orc)


@pytest.mark.gpu
def test_direct_route_inside_a_whole_call(ctxs):
    """the same select behind chicdiff_hip_wald_test_dev (size factors -> offsets -> fit in one enqueue)"""
    direct, classic = ctxs
    d = synth.make(50_000, 8)
    dk = direct.to_device(d["counts"], np.int32)
    dfm = direct.to_device(d["nf"] * (d["mu"][:, None] / 8), np.float64)
    want = ["dispersion", "log2FoldChange", "pvalue"]
    a, sa = direct.wald_test(dk, dfm, d["group"], theta=0.5, want=want)
    b, sb = classic.wald_test(dk, dfm, d["group"], theta=0.5, want=want)
    for k in want:
        assert np.array_equal(a[k].cpu().numpy(), b[k].cpu().numpy(), equal_nan=True), k
    assert np.array_equal(np.asarray(sa["sizeFactors"]), np.asarray(sb["sizeFactors"]))


@pytest.mark.gpu
def test_no_usable_row_is_the_same_error(ctxs):
    from chicdiff_amd import hip
    direct, classic = ctxs
    k = np.random.default_rng(2).poisson(20.0, size=(5000, 4)).astype(np.int32) + 1
    k[np.arange(5000), np.arange(5000) % 4] = 0  # every row holds a zero
    dk = direct.to_device(k, np.int32)
    msgs = []
    for c in (direct, classic):
        with pytest.raises(hip.ChicdiffHipError) as e:
            c.size_factors(dk)
        msgs.append(str(e.value))
    assert "every gene contains at least one zero" in msgs[0] and msgs[0] == msgs[1]
    # and the context is as good as before
    ok = synth.make(1001, 4)["counts"]
    assert np.array_equal(direct.size_factors(direct.to_device(ok, np.int32)), classic.size_factors(classic.to_device(ok, np.int32)))


@pytest.mark.gpu
def test_massive_ties_timed_on_both_routes(ctxs):
    """Allowed to be slow, not wrong.  One MI355X ("Variants measured"): 60 000 x 4 with 40 000 equal rows 0.288 ms
    per call on the direct route against 0.178 by the radix select; 18 000 x 4 of two values 0.145 against 0.171."""
    direct, classic = ctxs
    for name, counts in zip(("massive_ties", "two_tied_values"), tie_cases()):
        dk = direct.to_device(counts, np.int32)
        res = {}
        for tag, c in (("direct", direct), ("radix", classic)):
            c.size_factors(dk)
            t0 = time.perf_counter()
            for _ in range(10):
                res[tag] = c.size_factors(dk)
            print(f"{name} {tag}: {(time.perf_counter() - t0) / 10 * 1e3:.3f} ms per call (with its synchronisation)")
        assert np.array_equal(res["direct"], res["radix"]), name
