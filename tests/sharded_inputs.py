"""Deterministic inputs of the small sharded suite (tests/test_gpu_sharded_small.py; their preconditions: tests/test_sharded_inputs.py).

A case is a split (rows per rank), a design (S, group) and a content.  The whole matrix is built once and the ranks take consecutive
slices of it by the split's counts — the library takes any n per rank, so only one split comes from `shard_bounds`.

  split     rows per rank                    what it is there for
  w2        [1, 4099]                        a one-row rank in front of everything else
  w3        [2049, 63, 2048]                 one row more than a trend workgroup takes, less than a wave, exactly a workgroup
  w4        [64, 65, 1, 4000]                a wave, a wave + 1, one row, the rest
  w7        [1, 1, 1, 1, 1, 1, 4200]         a world that is no power of two; cnt < maxn on six of seven ranks
  w8        shard_bounds(4101, 8, r)         513 x 5, 512 x 3: the uneven split real use gives
  w5        [257, 255, 256, 129, 3300]       around the 128- and 256-row tiles

Content: `synth.make(total, S, fragments=2)` (counts; FullMean = the two fragments' sum, NaN rows included) with three rows zeroed,
then one planted variant:

  base            nothing more
  zero_shard      every row of one middle rank is all zero: no size-factor ratio, no trend row from that rank
  no_ratio_shard  every row of one rank has a zero in one sample: fitted, but the rank gives no candidate to the size-factor medians
  flat_shard      the counts of one rank's rows are round(c_i sf_j / gm(sf)) with c_i in [1500, 6000], FullMean c_i sf_j: the offsets of
                  such a row are sf / gm(sf), so the counts follow mu to +-0.5 where Poisson noise alone would be +-40 .. 80 — gene-wise
                  estimates at the floor, no row of the rank usable for the trend.  (sf: plain-numpy size factors of the matrix before
                  planting; the planted rows' own ratios sit on the medians, which therefore do not move by more than the rounding.)
  ties            one row (counts and FullMean) copied onto the first 56 % of every rank's rows, at least one per rank: more copies than
                  half of ALL rows, so the size-factor medians and the median of the trend's residuals land inside one run of equal keys
                  that has members on every rank (and the MAD is 0: more than half of the absolute deviations are 0)

`zero_rows=False` (the theta grid: its total deviance is NA as soon as one row is all zero) leaves no all-zero row: the three are not
planted and the generator's own get a count of 1 in every sample.
"""
import numpy as np

from chicdiff_amd import synth
from chicdiff_amd.dist import shard_bounds

SPLITS = {
    "w2": [1, 4099],
    "w3": [2049, 63, 2048],
    "w4": [64, 65, 1, 4000],
    "w7": [1, 1, 1, 1, 1, 1, 4200],
    "w8": [hi - lo for lo, hi in (shard_bounds(4101, 8, r) for r in range(8))],
    "w5": [257, 255, 256, 129, 3300],
}

# design name -> (S, group)
DESIGNS = {
    "S3": (3, [0, 0, 1]),         # 2 v 1: one residual degree of freedom, the prior matched by simulation
    "S4": (4, [0, 0, 1, 1]),      # 2 v 2: two
    "S5": (5, [0, 0, 1, 1, 1]),   # three
    "S8": (8, list(synth.groups(8))),
    "S9": (9, list(synth.groups(9))),
    "S16": (16, list(synth.groups(16))),
    "S17": (17, list(synth.groups(17))),   # past the fused offsets and the size-factor route of S <= 16
    "S3i": (3, [0, 0, 0]),        # design ~1, what the theta grid fits
}

# (split, design, variant, planted rank): every split, every design and every variant at least once.  (`ties` at S = 16 and 17 only: with
# more than half of the rows on one point the parametric trend of the S = 4 and S = 8 matrices does not converge — by the CPU oracle
# too — and the fit goes to the local substitute, which is not what these cases are about.)
CASES = [
    ("w2", "S8", "base", None),
    ("w3", "S3", "zero_shard", 1),
    ("w4", "S4", "no_ratio_shard", 1),
    ("w7", "S5", "base", None),
    ("w8", "S9", "flat_shard", 3),
    ("w5", "S16", "ties", None),
    ("w7", "S17", "ties", None),
    ("w3", "S3i", "base", None),
    ("w4", "S8", "zero_shard", 1),
    ("w5", "S9", "no_ratio_shard", 3),
    ("w8", "S4", "base", None),
    ("w2", "S17", "flat_shard", 0),
    ("w5", "S5", "flat_shard", 1),
]
UNEQUAL = [("w7", "S5", "base", None), ("w4", "S4", "no_ratio_shard", 1), ("w2", "S8", "base", None)]   # the variants' cases
GRID_CASES = [("w7", "S4", "base", None), ("w4", "S8", "base", None)]                                   # built with zero_rows=False
TIE_SHARE = 0.56
MIN_DISP = 1e-8   # chicdiff_hip_default_opts / oracle_nbglm_default_opts


def case_id(case):
    split, design, variant, _ = case
    return f"{split}-{design}-{variant}"


def bounds(split):
    """[(lo, hi)] per rank"""
    edges = np.concatenate([[0], np.cumsum(SPLITS[split])])
    return [(int(edges[r]), int(edges[r + 1])) for r in range(len(SPLITS[split]))]


def plain_size_factors(counts):
    """DESeq2's median of ratios in plain numpy — for planting only; nothing is compared with it"""
    ok = (counts > 0).all(axis=1)
    lg = np.log(counts[ok].astype(np.float64))
    return np.exp(np.median(lg - lg.mean(axis=1, keepdims=True), axis=0))


def tie_rows(split):
    """row indices that hold the copies of the `ties` variant"""
    idx = []
    for lo, hi in bounds(split):
        idx += list(range(lo, lo + max(1, int(np.ceil(TIE_SHARE * (hi - lo))))))
    return np.array(idx, dtype=np.int64)


_cache = {}


def build(case, zero_rows=True):
    """dict(counts (n, S) int32, fm (n, S) float64, group, S, split, bounds, variant, planted_rank, tie_rows | None, tie_source | None)"""
    key = (case, zero_rows)
    if key in _cache:
        return _cache[key]
    split, design, variant, planted = case
    S, group = DESIGNS[design]
    bnd = bounds(split)
    n = bnd[-1][1]
    d = synth.make(n, S, fragments=2)
    counts = d["counts"].copy()
    fm = d["fragFullMean"].reshape(n, 2, S).sum(axis=1)
    if zero_rows:
        counts[[n // 3, n // 2 + 1, n - 2]] = 0
    else:
        counts[counts.sum(axis=1) == 0] = 1
    out = dict(S=S, group=np.asarray(group, dtype=np.int32), split=split, bounds=bnd, variant=variant, planted_rank=planted,
               tie_rows=None, tie_source=None)
    if variant == "zero_shard":
        lo, hi = bnd[planted]
        counts[lo:hi] = 0
    elif variant == "no_ratio_shard":
        lo, hi = bnd[planted]
        rows = np.arange(lo, hi)
        counts[rows] = np.maximum(counts[rows], 1)   # (fitted: not all zero)
        counts[rows, rows % S] = 0
    elif variant == "flat_shard":
        lo, hi = bnd[planted]
        sf = plain_size_factors(counts)
        shape = sf / np.exp(np.log(sf).mean())
        c = 1500.0 + 4500.0 * ((np.arange(lo, hi) * 37) % 101) / 100.0
        counts[lo:hi] = np.rint(c[:, None] * shape[None, :]).astype(np.int32)
        fm[lo:hi] = c[:, None] * sf[None, :]
    elif variant == "ties":
        # the source: an ordinary row — every count positive, FullMean finite, a generating dispersion of 0.1 .. 0.4 at a mean of 20 .. 200
        good = (counts > 0).all(axis=1) & np.isfinite(fm).all(axis=1) & (d["alpha"] > 0.1) & (d["alpha"] < 0.4) & (d["mu"] > 20) & (d["mu"] < 200)
        good &= counts.std(axis=1) > 0.3 * counts.mean(axis=1)   # (visibly overdispersed in this very draw: an estimate far above the floor)
        src = int(np.flatnonzero(good)[0])
        rows = tie_rows(split)
        row_k, row_f = counts[src].copy(), fm[src].copy()
        counts[rows] = row_k
        fm[rows] = row_f
        out.update(tie_rows=rows, tie_source=(row_k, row_f))
    elif variant != "base":
        raise ValueError(variant)
    out.update(counts=np.ascontiguousarray(counts, dtype=np.int32), fm=np.ascontiguousarray(fm, dtype=np.float64))
    _cache[key] = out
    return out
