"""Inputs of the getCandidateInteractions tests: the reference's own regions with synthetic peaks, and small adversarial tables."""
import numpy as np

SCORE = 5.0


def _scores(rng, P, ncols=4, na=0.02):
    s = rng.lognormal(1.5, 1.0, size=(ncols, P))
    s[rng.random((ncols, P)) < na] = np.nan
    return s


def golden_case(golden, seed=7):
    """tests/golden/chr19_results.npz (24 863 regions, stored sorted by `group`, not by key): one peak per region at the middle of
    its range, 500 peaks 200-400 fragments beyond a real bait, deduplicated and shuffled; four log-normal score columns, 2 % NaN."""
    rng = np.random.default_rng(seed)
    b, lo, hi = (np.asarray(golden[k], dtype=np.int64) for k in ("baitID", "minOE", "maxOE"))
    far = rng.choice(np.unique(b), 500)
    pb = np.concatenate([b, far])
    po = np.concatenate([lo + (hi - lo) // 2, far + rng.integers(200, 401, 500)])
    pk = np.unique(np.stack([pb, po], axis=1), axis=0)
    pk = pk[rng.permutation(len(pk))]
    return dict(baitID=b.astype(np.int32), minOE=lo.astype(np.int32), maxOE=hi.astype(np.int32),
                peak_baitID=pk[:, 0].astype(np.int32), peak_oeID=pk[:, 1].astype(np.int32), scores=_scores(rng, len(pk)))


def adversarial_case(npeaks, nregions, seed, big_bait=False):
    """Spans 0..40 plus one region of span 300 placed first in its bait; tied regions (equal bait, minOE, maxOE, different p) copied
    both in front of and behind their originals; a negative baitID; with big_bait one bait of 3 000 regions and 70 regions stacked on
    one range (a peak of degree > 64).  Peaks at minOE, maxOE and maxOE + 1 of regions, in front of the first and behind the last
    key, on baits without regions; NaN p values; rows whose scores are all NaN; scores exactly at the threshold."""
    rng = np.random.default_rng(seed)
    nb = max(1, nregions // 30)
    baits = 1000 + 4000 * np.arange(1, nb + 1)
    if nregions >= 65:
        baits[0] = -7
    rb = rng.choice(baits, nregions)
    lo = rb + rng.integers(-400, 400, nregions)
    hi = lo + rng.integers(0, 41, nregions)
    if nregions >= 65:   # the wide region: the smallest minOE of its bait, far in front of the bait's other rows in key order
        w = int(rng.integers(nregions))
        lo[w] = rb[w] - 450
        hi[w] = lo[w] + 300
        for src, dst in ((3, 40), (50, 10), (20, 60), (61, 5)):   # ties, the copy behind and in front of the original
            rb[dst], lo[dst], hi[dst] = rb[src], lo[src], hi[src]
    if big_bait:
        rb = np.concatenate([rb, np.full(3000, 999000), np.full(70, 999000)])
        blo = 999000 + rng.integers(-2000, 2000, 3000)
        lo = np.concatenate([lo, blo, np.full(70, 999100)])
        hi = np.concatenate([hi, blo + rng.integers(0, 41, 3000), np.full(70, 999110)])
        perm = rng.permutation(len(rb))
        rb, lo, hi = rb[perm], lo[perm], hi[perm]
    n = len(rb)
    p = rng.random(n) ** 3
    p[rng.random(n) < 0.1] = np.nan
    deep = (rb == 999000) & (lo <= 999105) & (hi >= 999105)   # the regions of the degree > 64 peak: no NA, so that its group survives
    p[deep] = rng.random(int(deep.sum())) ** 3
    # peaks
    pick = rng.integers(0, n, 3 * npeaks + 8)
    kind = rng.integers(0, 4, len(pick))
    pb = rb[pick].copy()
    po = np.where(kind == 0, lo[pick], np.where(kind == 1, hi[pick], np.where(kind == 2, hi[pick] + 1, lo[pick] + (hi[pick] - lo[pick]) // 2)))
    extra_b = np.array([rb.min() - 3, rb.min(), rb.max(), rb.max() + 3, 555, 556, 999000])
    extra_o = np.array([5, lo.min() - 1, hi.max() + 1, 5, 600, 601, 999105])
    extra = np.stack([extra_b, extra_o], axis=1)[rng.permutation(len(extra_b))]
    rest = np.unique(np.stack([pb, po], axis=1), axis=0)
    rest = rest[~(rest[:, None, :] == extra[None, :, :]).all(axis=2).any(axis=1)]
    cand = np.concatenate([extra, rest[rng.permutation(len(rest))]])[:npeaks]   # the special peaks first: the cut never drops them all
    cand = cand[rng.permutation(len(cand))]
    if len(cand) < npeaks:   # baits without regions, all different
        k = npeaks - len(cand)
        cand = np.concatenate([cand, np.stack([9_000_000 + np.arange(k), np.arange(k)], axis=1)])
        cand = cand[rng.permutation(npeaks)]
    s = _scores(rng, npeaks, na=0.05)
    s[:, rng.random(npeaks) < 0.05] = np.nan
    at = np.flatnonzero(rng.random(npeaks) < 0.05)
    s[:, at] = np.array([SCORE, 1.0, 2.0, SCORE])[:, None]   # exactly the threshold: not selected
    s[:, (cand[:, 0] == 999000) & (cand[:, 1] == 999105)] = np.array([50.0, 60.0, 1.0, 2.0])[:, None]
    return dict(baitID=rb.astype(np.int32), minOE=lo.astype(np.int32), maxOE=hi.astype(np.int32), p=p,
                peak_baitID=cand[:, 0].astype(np.int32), peak_oeID=cand[:, 1].astype(np.int32), scores=s)


def twin_args(case, p, merged=False):
    """The case as the lists candidates_literal takes."""
    s = case["scores"]
    cols = ([0], [1]) if merged else (list(range(s.shape[0] // 2)), list(range(s.shape[0] // 2, s.shape[0])))
    return (case["baitID"].tolist(), case["minOE"].tolist(), case["maxOE"].tolist(), np.asarray(p, dtype=np.float64).tolist(),
            case["peak_baitID"].tolist(), case["peak_oeID"].tolist(), s.T.tolist(), cols[0], cols[1], merged)
