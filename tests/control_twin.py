"""numpy twin of the seeded control draws (chicdiff_hip_control_draws_dev), written from the rules of getControlRegionUniverse
(chicdiff.R:430-511) and the counter layout stated in include/chicdiff_hip.h — not from the kernels.

    philox4x32      Philox4x32-10 (Salmon et al. 2011), one block per (seed, k, attempt, stream)
    uniform         52 random bits + a half: u in [2^-53, 1 - 2^-53], exact in double
    qnorm           Wichura's AS 241 (PPND16) with numpy's log
    max_contact     max |baitID - otherEndID| per chromosome over RU ROWS (:463-464) — the yardstick for the kernel's region-level form
    control_draws   bait (:466-468), distance (giveDists, :434-444), seed of the region (giveOneSeed, :430-432), order (:480-481)
"""
import numpy as np

M0, M1 = np.uint64(0xD2511F53), np.uint64(0xCD9E8D57)
W0, W1 = 0x9E3779B9, 0xBB67AE85
MAX_ATTEMPTS = 256
_MASK = np.uint64(0xFFFFFFFF)


def philox4x32(c0, c1, c2, c3, k0, k1):
    """Ten rounds on arrays (or scalars) of 32-bit words; returns the four output words as uint64 arrays below 2^32."""
    c0, c1, c2, c3 = (np.atleast_1d(np.asarray(c, dtype=np.uint64)) & _MASK for c in (c0, c1, c2, c3))
    c0, c1, c2, c3 = np.broadcast_arrays(c0, c1, c2, c3)
    k0, k1 = int(k0) & 0xFFFFFFFF, int(k1) & 0xFFFFFFFF
    for _ in range(10):
        p0, p1 = M0 * c0, M1 * c2                                                  # 32 x 32 -> 64 bits: no overflow in uint64
        c0, c1, c2, c3 = (p1 >> np.uint64(32)) ^ c1 ^ np.uint64(k0), p1 & _MASK, (p0 >> np.uint64(32)) ^ c3 ^ np.uint64(k1), p0 & _MASK
        k0, k1 = (k0 + W0) & 0xFFFFFFFF, (k1 + W1) & 0xFFFFFFFF
    return c0, c1, c2, c3


def draw_words(seed, k, attempt, stream):
    """The block of draw k: key = (seed low, seed high), counter = (k low, k high, attempt, stream)."""
    seed = int(seed) & 0xFFFFFFFFFFFFFFFF
    k = np.asarray(k, dtype=np.uint64)
    return philox4x32(k & _MASK, k >> np.uint64(32), attempt, stream, seed & 0xFFFFFFFF, seed >> 32)


def uniform(r0, r1):
    r0, r1 = np.asarray(r0, dtype=np.uint64), np.asarray(r1, dtype=np.uint64)
    return ((r0 >> np.uint64(6)).astype(np.float64) * 67108864.0 + (r1 >> np.uint64(6)).astype(np.float64) + 0.5) * 2.0 ** -52


_A = [2509.0809287301226727, 33430.575583588128105, 67265.770927008700853, 45921.953931549871457, 13731.693765509461125,
      1971.5909503065514427, 133.14166789178437745, 3.387132872796366608]
_B = [5226.495278852545925, 28729.085735721942674, 39307.89580009271061, 21213.794301586595867, 5394.1960214247511077,
      687.1870074920579083, 42.313330701600911252, 1.0]
_C = [7.7454501427834140764e-4, 0.0227238449892691845833, 0.24178072517745061177, 1.27045825245236838258, 3.64784832476320460504,
      5.7694972214606914055, 4.6303378461565452959, 1.42343711074968357734]
_D = [1.05075007164441684324e-9, 5.475938084995344946e-4, 0.0151986665636164571966, 0.14810397642748007459, 0.68976733498510000455,
      1.6763848301838038494, 2.05319162663775882187, 1.0]
_E = [2.01033439929228813265e-7, 2.71155556874348757815e-5, 0.0012426609473880784386, 0.026532189526576123093, 0.29656057182850489123,
      1.7848265399172913358, 5.4637849111641143699, 6.6579046435011037772]
_F = [2.04426310338993978564e-15, 1.4215117583164458887e-7, 1.8463183175100546818e-5, 7.868691311456132591e-4, 0.0148753612908506148525,
      0.13692988092273580531, 0.59983220655588793769, 1.0]


def _horner(c, r):
    v = np.full_like(r, c[0])
    for x in c[1:]:
        v = v * r + x
    return v


def qnorm(p):
    """AS 241 for 0 < p < 1: a rational function of 0.180625 - q^2 in the middle, of sqrt(-log(tail)) outside."""
    p = np.atleast_1d(np.asarray(p, dtype=np.float64))
    q = p - 0.5
    out = np.empty_like(p)
    mid = np.abs(q) <= 0.425
    r = 0.180625 - q[mid] * q[mid]
    out[mid] = q[mid] * _horner(_A, r) / _horner(_B, r)
    t = ~mid
    r = np.sqrt(-np.log(np.where(q[t] < 0, p[t], 1.0 - p[t])))
    near = r <= 5.0
    v = np.empty_like(r)
    v[near] = _horner(_C, r[near] - 1.6) / _horner(_D, r[near] - 1.6)
    v[~near] = _horner(_E, r[~near] - 5.0) / _horner(_F, r[~near] - 5.0)
    out[t] = np.where(q[t] < 0, -v, v)
    return out


def max_contact(ru_baitID, ru_otherEndID, chr_of, nchr):
    """Row level, as the reference: max |baitID - otherEndID| over the RU rows whose bait is on chromosome c (0 = no row).
    ``chr_of[id]``: chromosome code of a restriction-map ID, -1 = not on the map (the merge of :463 drops such rows)."""
    b, o = np.asarray(ru_baitID, dtype=np.int64), np.asarray(ru_otherEndID, dtype=np.int64)
    code = np.asarray(chr_of)[b]
    out = np.zeros(nchr, dtype=np.int64)
    ok = code >= 0
    np.maximum.at(out, code[ok], np.abs(b - o)[ok])
    return out


def control_draws(seed, n_regions, bmap_id, bmap_chr, chr_min, chr_max, contact):
    """Draws k = 0 .. n_regions - 1.  ``bmap_chr``: the baitmap's chromosome in the map's code space (-1 = not on the map);
    ``contact``: max_contact().  Returns a dict: ``baitID, oeID`` the kept pairs sorted by (baitID, oeID); ``m``; per draw
    ``kept, draw_bait, draw_oe, attempts``; ``x``: per draw, the z * std of every attempt made."""
    bmap_id, bmap_chr = np.asarray(bmap_id, dtype=np.int64), np.asarray(bmap_chr, dtype=np.int64)
    chr_min, chr_max, contact = (np.asarray(a, dtype=np.int64) for a in (chr_min, chr_max, contact))
    nb = len(bmap_id)
    k = np.arange(n_regions, dtype=np.uint64)
    r0, r1, _, _ = draw_words(seed, k, 0, 0)
    idx = np.array([((int(a) | (int(b) << 32)) * nb) >> 64 for a, b in zip(r0, r1)], dtype=np.int64)
    bait, code = bmap_id[idx], bmap_chr[idx]
    kept = code >= 0
    kept[kept] = contact[code[kept]] > 0                                           # bmap[chr %in% max_contacts$chr] (:468)
    lo, hi = chr_min[np.where(kept, code, 0)], chr_max[np.where(kept, code, 0)]
    std = contact[np.where(kept, code, 0)] / 3.0                                   # :472
    dist = np.zeros(n_regions, dtype=np.int64)
    attempts = np.zeros(n_regions, dtype=np.int64)
    xs = [[] for _ in range(n_regions)]
    todo = np.flatnonzero(kept)
    for attempt in range(MAX_ATTEMPTS):
        if len(todo) == 0:
            break
        w0, w1, _, _ = draw_words(seed, todo.astype(np.uint64), attempt, 1)
        x = qnorm(uniform(w0, w1)) * std[todo]
        d = np.rint(x).astype(np.int64)                                            # R's round(): ties to even
        ok = (d != 0) & ((bait[todo] + np.abs(d) < hi[todo]) | (bait[todo] - np.abs(d) > lo[todo]))
        for j, v in zip(todo, x):
            xs[j].append(float(v))
        attempts[todo] = attempt + 1
        dist[todo[ok]] = d[ok]
        todo = todo[~ok]
    if len(todo):
        raise ValueError(f"draw {todo[0]}: bait {bait[todo[0]]} still rejected after {MAX_ATTEMPTS} attempts")
    fwd = bait + dist
    oe = np.where((fwd < lo) | (fwd > hi), bait - dist, fwd)                       # giveOneSeed: not strict
    order = np.lexsort((oe[kept], bait[kept]))
    return dict(baitID=bait[kept][order].astype(np.int32), oeID=oe[kept][order].astype(np.int32), m=int(kept.sum()), kept=kept,
                draw_bait=bait, draw_oe=oe, draw_chr=code, attempts=attempts, x=xs, reflected=kept & (oe != fwd))


def rounding_band(xs):
    """Draws with an attempt whose x lies within 2^-40 max(1, |x|) of a half-integer: only there could a last-bit difference of
    the logarithm turn the rounding."""
    out = []
    for j, v in enumerate(xs):
        if len(v):
            a = np.asarray(v)
            if (np.abs(np.abs(a - np.floor(a)) - 0.5) <= 2.0 ** -40 * np.maximum(1.0, np.abs(a))).any():
                out.append(j)
    return out
