"""Filler waves of the gene-wise line search (chicdiff_amd/csrc/disp_kernels.hip: "front waves and fillers"; common.h: queue_claim,
filler_claims).

With "line_search_fillers" on, the launch's two waves per SIMD run at issue priority and a third wave per SIMD takes chunks from the END
of the schedule only (rows of score >= 3.16, which are never long).  That decides WHEN and BY WHOM a row is searched, never a bit of its
result.  The claim rule of the two-ended queue is a plain function of (queue word, chunks), compiled for the host as well
(chicdiff_hip_selftest_queue_claim): the CPU part drives it through every interleaving of a few front and filler waves; the GPU part
compares whole fits with fillers off and on at the shapes where the two ends of the queue meet."""
import ctypes as C

import numpy as np
import pytest

from chicdiff_amd import synth

MIN_DISP = 1e-8
MINDISP_SLOT = 17  # classes above it: score >= 3.16 (tests/test_schedule_classes.py)
WANT = ["dispGeneEst", "dispGeneIter", "dispMAP", "dispersion", "log2FoldChange", "pvalue"]


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as g
    g.build()
    from chicdiff_amd import hip
    return hip.load_library()


# ---- CPU: the claim rule ----------------------------------------------------------------------------------------------------------------

def claim(L, old, back, chunks, first_back, stop, claimed=1):
    """the library's rule: (valid, chunk, may a filler that saw `old` claim again)"""
    chunk, again = C.c_uint32(0), C.c_int32(0)
    valid = L.chicdiff_hip_selftest_queue_claim(old, int(back), chunks, first_back, stop, int(claimed), C.byref(chunk), C.byref(again))
    return bool(valid), int(chunk.value), bool(again.value)


def stop_f(stop, chunks, first_back):
    """restated: the front counter at which fillers stop claiming — the share of the front's own chunks [0, first_back), rounded up"""
    if stop >= 100:
        return None
    return -(-min(first_back, chunks) * stop // 100)


def test_claim_names_chunks_from_both_ends(lib):
    for chunks in (0, 1, 2, 7, 1000):
        for f in range(0, chunks + 3):
            for b in range(0, chunks + 3):
                old = (b << 32) | f
                for back in (False, True):
                    valid, chunk, _ = claim(lib, old, back, chunks, 0, 100)
                    assert valid == (f + b < chunks)
                    if valid:
                        assert chunk == (chunks - 1 - b if back else f)
    # the halves do not run into each other: a front counter far beyond any chunk count leaves the back counter alone
    assert claim(lib, (3 << 32) | 0xfffffff0, True, 10, 0, 100)[0] is False


@pytest.mark.parametrize("n_front,n_fill", [(1, 1), (2, 1), (1, 2), (2, 2), (1, 3)])
def test_every_interleaving_hands_out_every_chunk_once(lib, n_front, n_fill):
    """Front waves claim until a claim is invalid; a filler claims while the rule lets it.  Every order in which their atomics can reach
    the queue word: each chunk exactly once, every valid claim worked, no filler claim after it has seen the boundary or the stop share."""
    for chunks in (0, 1, 2, 3, 5):
        for first_back in sorted({0, 1, chunks // 2, max(chunks - 1, 0), chunks, chunks + 1}):
            for stop in (0, 50, 100):
                sf = stop_f(stop, chunks, first_back)
                seen_states = set()
                leaves = 0
                # wave state: (alive, claimed, last old word); fronts first
                start = (0, tuple((True, False, 0) for _ in range(n_front + n_fill)), ())
                stack = [start]
                while stack:
                    state = stack.pop()
                    if state in seen_states:
                        continue
                    seen_states.add(state)
                    word, waves, worked = state
                    alive = [i for i, w in enumerate(waves) if w[0]]
                    if not alive:
                        leaves += 1
                        assert sorted(worked) == list(range(chunks)), (chunks, first_back, stop, worked)
                        continue
                    for i in alive:
                        _, claimed, last = waves[i]
                        back = i >= n_front
                        ws = list(waves)
                        if back:
                            again = claim(lib, last, True, chunks, first_back, stop, claimed)[2]
                            # the rule, restated: never when there is no filler region or the share of the front's own chunks comes to
                            # none (share 0, or no chunk in front of the boundary unless the share is 100 = never); after a claim only if
                            # that claim was valid, its chunk lay behind the boundary chunk and the front counter it saw was below the share
                            if claimed:
                                f, b = last & 0xffffffff, last >> 32
                                want = first_back < chunks and f + b < chunks and chunks - 1 - b > first_back and (sf is None or f < sf)
                            else:
                                want = first_back < chunks and (sf is None or sf > 0)
                            assert again == want, (chunks, first_back, stop, claimed, hex(last))
                            if not again:  # finishes its live rows and leaves: no atomic, nothing waits
                                ws[i] = (False, claimed, last)
                                stack.append((word, tuple(ws), worked))
                                continue
                        valid, chunk, _ = claim(lib, word, back, chunks, first_back, stop)
                        new_word = word + ((1 << 32) if back else 1)
                        new_worked = worked
                        if valid:
                            assert chunk not in worked and 0 <= chunk < chunks
                            new_worked = tuple(sorted(worked + (chunk,)))  # a valid claim is always worked by the wave that made it
                        ws[i] = (valid or back, True, word) if back else (valid, True, word)
                        stack.append((new_word, tuple(ws), new_worked))
                assert leaves > 0
    # fillers overshoot the boundary by at most one chunk per wave: a filler that worked a chunk <= first_back never claimed again (asserted
    # above through `want`), so the chunks in front of first_back that fillers worked are at most n_fill


def test_stop_share_is_a_share_of_the_front_waves_own_chunks(lib):
    chunks, first_back = 1000, 600
    for stop, f_stop in ((0, 0), (1, 6), (50, 300), (99, 594)):
        for f in (0, f_stop - 1, f_stop, f_stop + 1):
            if f < 0:
                continue
            again = claim(lib, (5 << 32) | f, True, chunks, first_back, stop)[2]
            assert again == (stop > 0 and f < f_stop), (stop, f)
    assert claim(lib, (5 << 32) | 990, True, chunks, first_back, 100)[2]  # 100 = never: the front counter may be anywhere
    assert not claim(lib, (400 << 32) | 10, True, chunks, first_back, 100)[2]  # chunk 599: in front of the boundary — the one overshoot
    assert not claim(lib, (399 << 32) | 10, True, chunks, first_back, 100)[2]  # chunk 600 IS the boundary chunk: nothing behind it to take
    assert claim(lib, (398 << 32) | 10, True, chunks, first_back, 100)[2]
    assert not claim(lib, 0, True, chunks, chunks, 100, claimed=0)[2]  # no chunk lies wholly in the filler region
    assert claim(lib, 0, True, chunks, first_back, 100, claimed=0)[2]


# ---- GPU: fillers never decide a bit ---------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def ctx():
    import __graft_entry__ as g
    g.build()
    from chicdiff_amd import hip
    c = hip.HipContext(0)
    yield c
    c.close()


def start_scores(counts, group):
    """alpha_init and the schedule score of every row of a matrix with offsets 1 (then xim = 1 whatever the rows): DESeq2's rough and
    moments estimates as disp_init_kernel forms them"""
    q = counts.astype(np.float64)
    S = q.shape[1]
    g = np.asarray(group) == 1
    bm, bv = q.mean(1), q.var(1, ddof=1)
    g0, g1 = q[:, ~g].mean(1), q[:, g].mean(1)
    m = np.where(g[None, :], np.maximum(g1, 1.0)[:, None], np.maximum(g0, 1.0)[:, None])
    with np.errstate(divide="ignore", invalid="ignore"):
        rough = np.maximum((((q - m) ** 2 - m) / m ** 2).sum(1) / (S - 2), 0.0)
        moments = (bv - bm) / bm ** 2
    a0 = np.minimum(np.maximum(MIN_DISP, np.minimum(rough, moments)), max(10.0, float(S)))
    return a0, a0 * np.minimum(g0, g1)


def crafted(kind, S, lib):
    """(counts, nf, group) of a fit of 70 000 rows — more than the 65 536 below which the search runs in natural order, fewer than the
    131 072 lanes of the front waves — whose schedule has the wanted shape; offsets are 1, so a row's class does not depend on the others"""
    n = 70000
    group = synth.groups(S)
    rng = np.random.default_rng([20260101, S, sum(map(ord, kind))])
    pool = synth.make(4 * n, S)["counts"]
    a0, score = start_scores(pool, group)
    live = pool.sum(1) > 0
    low = np.flatnonzero(live & (a0 > 1e-6) & (score < 0.2))     # dealt out statically whatever the order (score < 0.316, not a minDisp start)
    mid = np.flatnonzero(live & (score < 2.5))                   # in front of the boundary, minDisp starts included
    high = np.flatnonzero(live & (a0 > 1e-6) & (score > 5.0))    # the filler waves' end of the queue
    assert len(low) >= 3000 and len(mid) >= n and len(high) >= 3000
    if kind == "none_high":
        rows = pool[mid[:n]]
    elif kind == "all_high":
        rows = pool[rng.choice(high, n)]
    else:  # 3 000 dealt rows + K rows in the queue, all of them high; the rest of the matrix all zero (never scheduled)
        k = {"one_chunk": 50, "two_chunks": 100}[kind]
        rows = np.zeros((n, S), dtype=np.int32)
        rows[:3000] = pool[low[:3000]]
        rows[3000:3000 + k] = pool[high[:k]]
    rows = np.ascontiguousarray(rows[rng.permutation(n)])
    # the shape it was built for, by the library's own class function
    a0, score = start_scores(rows, group)
    livem = rows.sum(1) > 0
    cls = np.zeros(int(livem.sum()), dtype=np.int32)
    dp, ip = C.POINTER(C.c_double), C.POINTER(C.c_int32)
    gmin = np.ascontiguousarray(score[livem] / a0[livem])
    a0l = np.ascontiguousarray(a0[livem])
    assert lib.chicdiff_hip_selftest_sched_class(1, MIN_DISP, a0l.ctypes.data_as(dp), gmin.ctypes.data_as(dp), len(cls), cls.ctypes.data_as(ip), None) == 0
    behind = int((cls > MINDISP_SLOT).sum())
    if kind == "none_high":
        assert behind == 0
    elif kind == "all_high":
        assert behind == len(cls) == n
    else:
        assert behind == {"one_chunk": 50, "two_chunks": 100}[kind] and int((cls < 9).sum()) == 3000 == len(cls) - behind
    return rows, np.ones((n, S)), group


@pytest.mark.gpu
@pytest.mark.parametrize("S", [4, 8, 16])
@pytest.mark.parametrize("kind", ["few_rows", "none_high", "all_high", "one_chunk", "two_chunks", "many_rows"])
def test_fillers_off_and_on_agree_bit_for_bit(ctx, lib, kind, S):
    if kind == "few_rows":       # fewer rows than front lanes
        d = synth.make(70000, S)
        counts, nf, group = d["counts"], d["nf"], d["group"]
    elif kind == "many_rows":    # every front lane busy and rows to spare: front waves and fillers really race for the chunks in the middle
        d = synth.make(300000, S)
        counts, nf, group = d["counts"], d["nf"], d["group"]
    else:
        counts, nf, group = crafted(kind, S, lib)
    group = np.asarray(group, dtype=np.int32)
    dk, dn = ctx.to_device(counts, np.int32), ctx.to_device(nf, np.float64)

    def run():
        out, _ = ctx.nbglm_fit(dk, dn, group, want=WANT)
        return {k: out[k].cpu().numpy().copy() for k in WANT}

    try:
        ctx.set_option("line_search_fillers", 0)
        ref = run()
        assert np.isfinite(ref["dispGeneEst"]).sum() >= 3000
        # one and two chunks: everything in front of the minDisp starts dealt out statically, so that the queue holds the 50 / 100 rows alone
        classes_a = 5 if kind in ("one_chunk", "two_chunks") else 0
        ctx.set_option("line_search_classes_a", classes_a)
        for schedule in (1, 3, 4, 0):
            ctx.set_option("line_search_schedule", schedule)
            for fillers, stop in ((0, 100), (1, 0), (1, 50), (1, 100), (-1, -1)):
                if fillers == 0 and schedule == 1 and classes_a == 0:
                    continue
                ctx.set_option("line_search_fillers", fillers)
                ctx.set_option("line_search_filler_stop", stop)
                got = run()
                for k in WANT:
                    differ = int((~((got[k] == ref[k]) | (np.isnan(got[k]) & np.isnan(ref[k])))).sum())
                    print(f"{kind} S {S} schedule {schedule} fillers {fillers} stop {stop} {k}: rows that differ {differ}")
                    assert np.array_equal(got[k], ref[k], equal_nan=True), (kind, S, schedule, fillers, stop, k, differ)
    finally:
        ctx.set_option("line_search_schedule", 1)
        ctx.set_option("line_search_classes_a", 0)
        ctx.set_option("line_search_fillers", -1)
        ctx.set_option("line_search_filler_stop", -1)
