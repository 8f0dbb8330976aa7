"""Schedule of the gene-wise line search (chicdiff_amd/csrc/common.h: sched_class; disp_kernels.hip: order_*).

The schedule decides WHEN a row is visited, never a bit of its result: the 1/8-decade order (default), the same with the
minDisp starts last, the six half-decade classes of earlier releases and the natural row order must give identical
fits, with either build of the search kernel (two or three waves per SIMD).  The class function itself runs on the host too
(chicdiff_hip_selftest_sched_class), so its shape is checked without a GPU against a numpy restatement."""
import ctypes as C

import numpy as np
import pytest

from chicdiff_amd import synth

MIN_DISP = 1e-8
# 10^(k/8), k = -12 .. 8, to four digits — except the half-decades, which are the literals the six-class order has always used
EDGES = np.array([0.0316, 0.0422, 0.0562, 0.0750, 0.1, 0.1334, 0.1778, 0.2371, 0.316, 0.4217, 0.5623, 0.7499, 1.0,
                  1.3335, 1.7783, 2.3714, 3.16, 4.2170, 5.6234, 7.4989, 10.0])
N_CLASSES, MINDISP_SLOT = 23, 17


def np_sched_class(a0, gmin, min_disp, mode):
    """numpy restatement: class = number of edges not above the score, one index (17) left free for the minDisp starts"""
    a0, gmin = np.asarray(a0, dtype=np.float64), np.asarray(gmin, dtype=np.float64)
    s = a0 * gmin
    edges = EDGES[4::4] if mode == 3 else EDGES
    f = np.searchsorted(edges, s, side="right")
    if mode == 3:
        f = np.where(f > 0, 4 * f + 1, 0)  # a half-decade class sits at the index of its first 1/8-decade step
    c = np.where(f < MINDISP_SLOT, f, f + 1)
    at_min = ~(a0 > 1.5 * min_disp)
    return np.where(at_min, MINDISP_SLOT if mode in (1, 2) else N_CLASSES - 1, c).astype(np.int32)


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as g
    g.build()
    from chicdiff_amd import hip
    return hip.load_library()


def lib_sched_class(L, a0, gmin, mode):
    a0, gmin = np.ascontiguousarray(a0, dtype=np.float64), np.ascontiguousarray(gmin, dtype=np.float64)
    cls, bounds = np.zeros(len(a0), dtype=np.int32), np.zeros(7, dtype=np.int32)
    dp, ip = C.POINTER(C.c_double), C.POINTER(C.c_int32)
    rc = L.chicdiff_hip_selftest_sched_class(mode, MIN_DISP, a0.ctypes.data_as(dp), gmin.ctypes.data_as(dp), len(a0),
                                             cls.ctypes.data_as(ip), bounds.ctypes.data_as(ip))
    assert rc == 0
    return cls, bounds


def scores():
    rng = np.random.default_rng(7)
    s = np.concatenate([10.0 ** rng.uniform(-4, 3, 20000), EDGES, np.nextafter(EDGES, 0), np.nextafter(EDGES, np.inf), [0.0, 1e-300, 1e300]])
    return np.sort(s)


@pytest.mark.parametrize("mode", [1, 3, 4])
def test_class_is_monotone_in_the_score_and_matches_numpy(lib, mode):
    s = scores()
    # the score is alpha_init * (smaller group mean): put it on either factor
    for a0, gmin in ((np.ones_like(s), s), (np.maximum(s, 1e-6), s / np.maximum(s, 1e-6))):
        cls, _ = lib_sched_class(lib, a0, gmin, mode)
        order = np.argsort(a0 * gmin, kind="stable")
        assert np.all(np.diff(cls[order]) >= 0), "a higher score must never be visited earlier"
        assert np.array_equal(cls, np_sched_class(a0, gmin, MIN_DISP, mode))
        assert cls.min() >= 0 and cls.max() == N_CLASSES - 1
    if mode != 3:  # about 1/8 decade per class between 0.0316 and 10: every one of the twenty steps is used
        cls, _ = lib_sched_class(lib, np.ones_like(s), s, mode)
        used = set(np.unique(cls))
        assert used == set(range(N_CLASSES)) - {MINDISP_SLOT}
        lo, hi = EDGES[:-1], EDGES[1:]
        assert np.all(np.abs(np.log10(hi / lo) - 0.125) < 2e-3)


def test_mindisp_starts_go_last_or_in_front_of_the_high_scores(lib):
    a0 = np.array([MIN_DISP, 1.5 * MIN_DISP, 1.4e-8, 2e-8, 1e-3])
    gmin = np.array([5.0, 1e9, 100.0, 1e9, 1e3])
    for mode, want in ((1, MINDISP_SLOT), (3, N_CLASSES - 1), (4, N_CLASSES - 1)):
        cls, _ = lib_sched_class(lib, a0, gmin, mode)
        assert list(cls[:3]) == [want] * 3
        assert cls[3] == N_CLASSES - 1 and cls[4] == 13  # score 20 (>= 10) and score 1.0 (first step of [1, 3.16))
        assert np.array_equal(cls, np_sched_class(a0, gmin, MIN_DISP, mode))
    # by default every class behind the minDisp starts holds scores >= 3.16 only
    s = scores()
    cls, _ = lib_sched_class(lib, np.ones_like(s), s, 1)
    assert s[cls > MINDISP_SLOT].min() >= 3.16 and s[cls < MINDISP_SLOT].max() < 3.16


@pytest.mark.parametrize("mode", [1, 3, 4])
def test_static_deal_boundary_has_not_moved(lib, mode):
    """The static deal takes the classes below a half-decade edge of the score (by default the first two of six: score < 0.316).
    Whatever the order's grain, the rows on either side of each such boundary are the rows the six-class order had there."""
    s = scores()
    a0 = np.ones_like(s)
    cls, bounds = lib_sched_class(lib, a0, s, mode)
    six = np.select([s < 0.1, s < 0.316, s < 1.0, s < 3.16, s < 10.0], [0, 1, 2, 3, 4], 5)  # the six-class order, restated
    assert bounds[0] == 0 and bounds[6] == N_CLASSES
    for a in range(1, 5):
        assert np.array_equal(cls < bounds[a], six < a), (mode, a)
    assert np.array_equal(cls < bounds[2], s < 0.316)  # the default deal
    # five classes = all but the last, where the minDisp starts and the scores >= 10 are (default order: all in front of the minDisp starts)
    at_min = np.full(4, MIN_DISP)
    cls_min, _ = lib_sched_class(lib, at_min, np.array([0.01, 1.0, 5.0, 50.0]), mode)
    assert np.all(cls_min >= bounds[5])
    if mode != 1:
        assert np.array_equal(cls < bounds[5], six < 5)
    else:
        assert np.array_equal(cls < bounds[5], six < 4)


# ---- GPU: the order never decides a bit ---------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def ctx():
    import __graft_entry__ as g
    g.build()
    from chicdiff_amd import hip
    c = hip.HipContext(0)
    yield c
    c.close()


@pytest.mark.gpu
@pytest.mark.parametrize("n,S", [(250000, 8), (70000, 4), (150000, 16)])
def test_schedules_agree_bit_for_bit(ctx, n, S):
    d = synth.make(n, S)
    group = np.asarray(d["group"], dtype=np.int32)
    dk, dn = ctx.to_device(d["counts"], np.int32), ctx.to_device(d["nf"], np.float64)
    want = ["dispGeneEst", "dispGeneIter", "dispMAP", "dispersion", "log2FoldChange", "pvalue"]

    def run():
        out, _ = ctx.nbglm_fit(dk, dn, group, want=want)
        return {k: out[k].cpu().numpy().copy() for k in want}

    ref = run()  # the default: 1/8-decade classes, waves per SIMD by the launcher's rule
    assert np.isfinite(ref["dispGeneEst"]).sum() > n // 2 and ref["dispGeneIter"].max() >= 50, "the matrix must hold long rows"
    try:
        for waves in (0, 2, 3):
            ctx.set_option("line_search_min_waves", waves)
            for schedule in (1, 3, 0, 4):
                if waves == 0 and schedule == 1:
                    continue
                ctx.set_option("line_search_schedule", schedule)
                got = run()
                for k in want:
                    differ = int((~((got[k] == ref[k]) | (np.isnan(got[k]) & np.isnan(ref[k])))).sum())
                    print(f"{n} x {S} min_waves {waves} schedule {schedule} {k}: rows that differ {differ}")
                    assert np.array_equal(got[k], ref[k], equal_nan=True), (k, waves, schedule, differ)
    finally:
        ctx.set_option("line_search_schedule", 1)
        ctx.set_option("line_search_min_waves", 0)
