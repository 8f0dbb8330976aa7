"""Small inputs that reach every path of the Wald stage (tests/test_wald_twin.py, tests/test_gpu_wald.py).

One case per design, 599 rows each: two full 256-thread blocks and a partial wave.  Rows come from synth.make; the fit runs with
trendCoef = (0.05, 2.0) and dispPriorVar = 1.0 given, so no trend is fitted, nothing is simulated and a case costs milliseconds.

Planted in every ~condition case (row positions in `case["planted"]`):
  slow    offsets spread log-uniformly over 0.05 .. 20, group B all zero but for a few counts of 1 .. 2 (one for a cell of up to five
          samples, a third of the cell beyond; every fifth row: none): some mu of the cell sit at the 0.5 floor and some do not, and
          the IRLS takes up to 99 steps;
  bzero   group B all zero: every mu of the cell ends at the floor, where the deviance no longer moves — these rows stop after two to
          four steps, with every weight of the cell a floored one (they do NOT reach the optimiser: the floor keeps beta inside 30);
  huge    one count of 2 000 * 2^k, k = 0 .. 10: from 16 000 or so on the IRLS runs to 100 steps and the row goes to the optimiser;
  tie     offsets == 1 and repeated counts, so that the largest Cook's distance is taken by two or more samples with EXACTLY equal
          values (identical samples of one cell).  Where cell B has four samples or more: B = (c + d, c + d, c - d, c - d, c, ...), the
          residuals of a cell sum to zero, so a pair is on top.  In a cell of three, two equal samples can never be on top (the third
          one's residual is twice theirs): there, and in some rows of every case, both cells are constant, every residual is the
          ridge's 1e-7 and every sample of a cell has the same distance — the rows that also make a cell's trimmed mean a matter of
          WHICH equal values are dropped;
  zero    three all-zero rows;
  copies  eight of the rows above again at the first, at a middle and at the last row positions.
"""
import numpy as np

from chicdiff_amd import synth

N = 599
SEED = 2400  # chosen (tests/test_wald_twin.py asserts what it was chosen for): every case gets its slow rows, none a stop at the tolerance
OPTS = dict(trendCoef=(0.05, 2.0), dispPriorVar=1.0)
N_SLOW, N_BZERO, N_HUGE, N_TIE = 48, 16, 16, 12


def _group(spec, S):
    if spec == "halves":
        return synth.groups(S)
    return np.array([int(c) for c in spec], dtype=np.int32)


# name -> (S, group, what it reaches)
DESIGNS = {
    "S4-0011": (4, "0011", "no cell of 3: maxCooks NaN, arg-max -1"),
    "S5-00111": (5, "00111", "one cell counts for the maximum; the arg-max runs over all samples"),
    "S6-010101": (6, "010101", "interleaved group mask; the n = 3 trim class"),
    "S8-4v4": (8, "halves", "scale 1.86, one value dropped at each end"),
    "S15-7v8": (15, "halves", "one value dropped (cell of 7) and two (cell of 8) in one row"),
    "S47-23v24": (47, "halves", "both sides of the 23.5 class edge (5 and 3 values dropped)"),
    "S64-32v32": (64, "halves", "top bit of the 64-bit mask, 4 values dropped"),
    "S3-intercept": (3, "000", "design ~1"),
    "S8-intercept": (8, "00000000", "design ~1"),
}
CONDITION_CASES = [k for k in DESIGNS if "intercept" not in k]
INTERCEPT_CASES = [k for k in DESIGNS if "intercept" in k]
_cache = {}


def make_case(name):
    if name in _cache:
        return _cache[name]
    S, spec, what = DESIGNS[name]
    group = _group(spec, S)
    d = synth.make(N, S)
    counts, nf = d["counts"].copy(), d["nf"].copy()
    rng = np.random.default_rng(SEED + S)
    A, B = np.flatnonzero(group == 0), np.flatnonzero(group == 1)
    planted = {}
    pos = 8
    if len(B):
        rows = np.arange(pos, pos + N_SLOW)
        for t, i in enumerate(rows):
            nf[i] = np.exp(rng.uniform(np.log(0.05), np.log(20.0), S))
            counts[i, A] = rng.poisson(20.0 * nf[i, A])
            counts[i, A[0]] = max(counts[i, A[0]], 1)
            counts[i, B] = 0
            if t % 5:
                m = max(1, len(B) // 3)
                counts[i, rng.choice(B, m, replace=False)] = 1 + rng.integers(0, 2, m)
        planted["slow"] = rows
        pos += N_SLOW
        rows = np.arange(pos, pos + N_BZERO)
        for i in rows:
            counts[i, A] = np.maximum(counts[i, A], 1)
            counts[i, B] = 0
        planted["bzero"] = rows
        pos += N_BZERO
        rows = np.arange(pos, pos + N_HUGE)
        for t, i in enumerate(rows):
            counts[i, 0] = max(counts[i, 0], 1)
            counts[i, rng.integers(0, S)] = 2000 * 2 ** (t % 11)
        planted["huge"] = rows
        pos += N_HUGE
        rows = np.arange(pos, pos + N_TIE)
        for t, i in enumerate(rows):
            nf[i] = 1.0
            a, c, dd = 12 + 5 * t, 40 + 7 * t, 9 + 2 * t
            counts[i, A] = a
            counts[i, B] = c
            if len(B) >= 4 and t % 3:  # two pairs at +- d around the cell's mean
                counts[i, B[0]] = counts[i, B[1]] = c + dd
                counts[i, B[2]] = counts[i, B[3]] = c - dd
        planted["tie"] = rows
        pos += N_TIE
    else:
        rows = np.arange(pos, pos + N_HUGE)
        for t, i in enumerate(rows):
            counts[i, rng.integers(0, S)] = 2000 * 2 ** (t % 11)
        planted["huge"] = rows
        pos += N_HUGE
    rows = np.arange(pos, pos + 3)
    counts[rows] = 0
    planted["zero"] = rows
    pos += 3
    hard = np.concatenate([planted[k][:2] for k in ("slow", "bzero", "huge", "tie") if k in planted])
    if len(hard) < 8:
        hard = np.concatenate([hard, np.arange(pos, pos + 8 - len(hard))])
    copies = [np.arange(0, 8), np.arange(N // 2 - 4, N // 2 + 4), np.arange(N - 8, N)]
    for dst in copies:
        counts[dst], nf[dst] = counts[hard], nf[hard]
    planted["hard"] = hard
    planted["copies"] = np.stack(copies)  # copies[k, t] is a copy of hard[t]
    assert pos <= N // 2 - 4
    case = dict(name=name, S=S, group=group, counts=np.ascontiguousarray(counts, dtype=np.int32), nf=np.ascontiguousarray(nf), planted=planted,
                what=what, two_groups=bool(len(B)), opts=dict(OPTS))
    _cache[name] = case
    return case
