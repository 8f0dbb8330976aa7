"""The region stage, restated from chicdiff.R with Python integers, dicts and fractions.Fraction: the twin that
tests/test_region_twin.py holds against the CPU oracle and tests/test_gpu_region.py against the device.  It imports nothing from
chicdiff_amd or oracle and shares no expression with either; where an input is too large for the statement-by-statement form there is
a numpy form beside it, and tests/test_region_twin.py holds the two equal on every small case.

  region universe     chicdiff.R:353-426   region_universe, region_universe_np          (the rows themselves: post_inputs.region_universe_literal)
  bait filter, keys   :826-831, :849       key_table, key_table_np
  join                :843-858             join_left           merge(x, temp, all.x = TRUE); N[is.na(N)] <- 0
  no-chinput branch   :774-807             join_inner          Reduce(merge, tempForCounts), then the left join
  avDist              :868-882, :1965-1967 avdist, avdist_long_double
"""
from fractions import Fraction

import numpy as np

from post_inputs import region_universe_literal

INT32_MIN, INT32_MAX = -2 ** 31, 2 ** 31 - 1
NA_INT = INT32_MIN  # what the entry points write for an empty region's minOE / maxOE


# ---- region universe (chicdiff.R:353-426) -------------------------------------------------------------------------------
def window(bait, oe, s, maxfrag=None):
    """.expandAvoidBait(bait, oe, s) (:353-367) as (lo, hi) of the set R's a:b holds (it counts down when a > b), in Python integers;
    None for bait == oe (the stop()).  With ``maxfrag`` the window is clamped to [1, maxfrag] and an empty one is (1, 0)."""
    bait, oe, s = int(bait), int(oe), int(s)
    if abs(bait - oe) > s + 1:
        a, e = oe - s, oe + s
    elif oe > bait:
        a, e = bait + 2, oe + s
    elif oe < bait:
        a, e = oe - s, bait - 2
    else:
        return None
    lo, hi = min(a, e), max(a, e)
    if maxfrag is not None:
        lo, hi = max(lo, 1), min(hi, int(maxfrag))
        if lo > hi:
            lo, hi = 1, 0
    return lo, hi


def region_universe(bait, oe, s, chr_of):
    """What the device returns for getRegionUniverse: RU.DT's rows (region_universe_literal: chicdiff.R:353-401 statement by
    statement) put in (regionID, otherEndID) order, their CSR offsets and each region's smallest / largest otherEndID (NA_INT for an
    empty region).  Raises ValueError("Invalid parameters") for baitID == oeID, as the literal form does."""
    lit = region_universe_literal(np.asarray(bait), np.asarray(oe), int(s), chr_of)
    rows = sorted(((int(r), int(o), int(b)) for b, r, o in lit.tolist()))   # (regionID, otherEndID, baitID)
    n = len(bait)
    per = [[] for _ in range(n)]
    for r, o, b in rows:
        per[r - 1].append(o)
    ptr = [0]
    for p in per:
        ptr.append(ptr[-1] + len(p))
    i32 = lambda v: np.array(v, dtype=np.int32).reshape(-1)
    return dict(region_ptr=np.array(ptr, dtype=np.int64), baitID=i32([b for _, _, b in rows]), regionID=i32([r for r, _, _ in rows]),
                otherEndID=i32([o for _, o, _ in rows]), minOE=i32([min(p) if p else NA_INT for p in per]),
                maxOE=i32([max(p) if p else NA_INT for p in per]))


def region_universe_np(bait, oe, s, chr_of):
    """The same in numpy (int64 throughout), for the one case too large for lists.  Raises like ``region_universe``."""
    b, o, s = np.asarray(bait, dtype=np.int64), np.asarray(oe, dtype=np.int64), int(s)
    chr_of = np.asarray(chr_of, dtype=np.int64)
    maxfrag = len(chr_of) - 1
    if np.any(b == o):
        raise ValueError("Invalid parameters")
    far = np.abs(b - o) > s + 1
    a = np.where(far | (o < b), o - s, b + 2)
    e = np.where(far | (o > b), o + s, b - 2)
    lo, hi = np.minimum(a, e), np.maximum(a, e)
    W = max(2 * s + 1, 2)
    assert int((hi - lo).max()) < W
    cand = lo[:, None] + np.arange(W, dtype=np.int64)[None, :]
    ok = (cand <= hi[:, None]) & (cand >= 1) & (cand <= maxfrag)
    cchr = np.where(ok, chr_of[np.where(ok, cand, 0)], -1)
    bok = (b >= 1) & (b <= maxfrag)
    bchr = np.where(bok, chr_of[np.where(bok, b, 0)], -1)
    keep = ok & (cchr >= 0) & (bchr[:, None] >= 0) & (cchr == bchr[:, None])
    cnt = keep.sum(axis=1)
    ptr = np.concatenate([[0], np.cumsum(cnt)]).astype(np.int64)
    reg, _ = np.nonzero(keep)                                                  # row-major: (regionID, otherEndID) order
    big = np.iinfo(np.int64).max
    mn = np.where(keep, cand, big).min(axis=1)
    mx = np.where(keep, cand, -big).max(axis=1)
    return dict(region_ptr=ptr, baitID=b[reg].astype(np.int32), regionID=(reg + 1).astype(np.int32), otherEndID=cand[keep].astype(np.int32),
                minOE=np.where(cnt > 0, mn, NA_INT).astype(np.int32), maxOE=np.where(cnt > 0, mx, NA_INT).astype(np.int32))


# ---- bait filter and key table (chicdiff.R:826-831, :849) -----------------------------------------------------------------
def pack(bait, oe):
    """(baitID, otherEndID) as the table's key stores it: baitID << 32 | the otherEndID's 32-bit pattern."""
    return (int(bait) << 32) | (int(oe) & 0xFFFFFFFF)


def key_table(bait, oe, N, flags=None):
    """x[J(baits)] (:828-831) and setkey(temp, baitID, otherEndID) (:849): a row is kept when bait >= 0 and, if ``flags`` (one per ID
    0 .. max_id) are given, when bait <= max_id and its flag is set; kept rows in STABLE order by key.  Returns (keys, vals)."""
    rows = []
    for b, o, v in zip(np.asarray(bait).tolist(), np.asarray(oe).tolist(), np.asarray(N).tolist()):
        if b < 0:
            continue
        if flags is not None and not (b <= len(flags) - 1 and flags[b]):
            continue
        rows.append((pack(b, o), v))
    rows.sort(key=lambda t: t[0])   # list.sort is stable
    return np.array([k for k, _ in rows], dtype=np.int64), np.array([v for _, v in rows], dtype=np.int32)


def key_table_np(bait, oe, N, flags=None):
    b, o, v = np.asarray(bait, dtype=np.int64), np.asarray(oe, dtype=np.int64), np.asarray(N, dtype=np.int32)
    keep = b >= 0
    if flags is not None:
        f = np.asarray(flags).astype(bool)
        inside = keep & (b <= len(f) - 1)
        keep = inside & f[np.where(inside, b, 0)]
    keys = (b[keep] << 32) | (o[keep] & 0xFFFFFFFF)
    order = np.argsort(keys, kind="stable")
    return keys[order], v[keep][order]


def table_dict(keys, vals):
    """A key table as {(baitID, otherEndID): N}, the pair as signed integers again.  Unique pairs only."""
    d = {}
    for k, v in zip(np.asarray(keys).tolist(), np.asarray(vals).tolist()):
        o = k & 0xFFFFFFFF
        pair = (k >> 32, o - (1 << 32) if o >= 1 << 31 else o)
        assert pair not in d, "the joins are defined for tables of unique pairs"
        d[pair] = v
    return d


# ---- joins ----------------------------------------------------------------------------------------------------------------
def join_left(qbait, qoe, table):
    """merge(x, temp, all.x = TRUE); x[is.na(N), N := 0] (:851-853): a dict look-up."""
    return np.array([table.get(q, 0) for q in zip(np.asarray(qbait).tolist(), np.asarray(qoe).tolist())], dtype=np.int32).reshape(-1)


def reduce_merge(dicts):
    """mergedFiles <- Reduce(merge, tempForCounts) (:778): merge()'s default, an INNER join on (baitID, otherEndID)."""
    merged = set(dicts[0])
    for d in dicts[1:]:
        merged &= set(d)
    return merged


def join_inner(qbait, qoe, dicts):
    """The no-chinput branch (:774-807): N (nru, S): a pair keeps its counts only when every replicate's table holds it."""
    merged = reduce_merge(dicts)
    out = np.zeros((len(qbait), len(dicts)), dtype=np.int32)
    for r, q in enumerate(zip(np.asarray(qbait).tolist(), np.asarray(qoe).tolist())):
        if q in merged:
            out[r] = [d[q] for d in dicts]   # merge(x, temp, all.x = TRUE); N[is.na(N)] <- 0
    return out


# ---- avDist (chicdiff.R:868-882, :1965-1967) ------------------------------------------------------------------------------
def _region_sums(ru_bait, ru_oe, region_ptr, id_min, midsum, chr_codes):
    """Per region: (sum of distSign, rows kept, any NA).  midpoint := round(0.5 * (start + end)) (:871; R's round is half to even,
    as Python's on a Fraction); merge() with rmap drops a row whose fragment the map lacks (:874-875; a chromosome code below zero =
    not on the map); distSign is NA for a trans row (:878-881)."""
    ms = [int(x) for x in np.asarray(midsum).tolist()]
    mid = [round(Fraction(x, 2)) for x in ms]
    ch = None if chr_codes is None else np.asarray(chr_codes).tolist()
    nid = len(ms)
    b, o, ptr = np.asarray(ru_bait).tolist(), np.asarray(ru_oe).tolist(), np.asarray(region_ptr).tolist()
    out = []
    for i in range(len(ptr) - 1):
        tot, cnt, na = 0, 0, False
        for r in range(ptr[i], ptr[i + 1]):
            ib, io = b[r] - id_min, o[r] - id_min
            if not (0 <= ib < nid and 0 <= io < nid):
                continue
            if ch is not None and (ch[ib] < 0 or ch[io] < 0):
                continue
            cnt += 1
            if ch is not None and ch[ib] != ch[io]:
                na = True
                continue
            tot += mid[io] - mid[ib]
        out.append((tot, cnt, na))
    return out


def avdist(ru_bait, ru_oe, region_ptr, id_min, midsum, chr_codes=None):
    """RU.recast[, list(avDist = mean(distSign)), by = "regionID"] (:1965-1967): mean() has no na.rm, so one NA row makes the region NA;
    an empty region, or one with every row dropped, is NaN.  The mean is the correctly rounded quotient of two integers."""
    return np.array([float("nan") if (na or cnt == 0) else float(Fraction(tot, cnt))
                     for tot, cnt, na in _region_sums(ru_bait, ru_oe, region_ptr, id_min, midsum, chr_codes)], dtype=np.float64).reshape(-1)


def avdist_long_double(ru_bait, ru_oe, region_ptr, id_min, midsum, chr_codes=None):
    """The same by data.table's route: gmean adds in long double, divides in long double, and the result is rounded to double."""
    out = []
    for tot, cnt, na in _region_sums(ru_bait, ru_oe, region_ptr, id_min, midsum, chr_codes):
        assert abs(tot) < 2 ** 53  # an integer that reaches the long double exactly, whichever way numpy converts it
        out.append(float("nan") if (na or cnt == 0) else float(np.longdouble(tot) / np.longdouble(cnt)))
    return np.array(out, dtype=np.float64).reshape(-1)
