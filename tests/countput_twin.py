"""numpy twin of countput for ONE condition, written from the rule above chicdiff_hip_countput_dev in include/chicdiff_hip.h (not from
pipeline._countput's text): rows kept, groups in order of first appearance, Kahan means in row order with the reset of a NaN
compensation, the strict maximum, the exact midpoint.  Whole-array numpy; the sequential recurrences run over the position inside
the group, all groups at once.

``compensated=False`` (the plain left-to-right sum) and ``reset=False`` (no ``c != c`` reset) are the rule's two neighbours: the tests
use them to show that their inputs can tell the rule from them."""
import numpy as np

COLUMNS = ("baitID", "otherEndID", "N", "Bmean", "score", "distSign")


def _sequential_mean(v, rows_at, sizes, compensated=True, reset=True):
    """Per group the mean of v over its rows in order: rows_at(p, live) = the row at position p of the groups ``live``."""
    G = len(sizes)
    s, c, cnt = np.zeros(G), np.zeros(G), np.zeros(G)
    with np.errstate(invalid="ignore", over="ignore"):
        for p in range(int(sizes.max()) if G else 0):
            live = np.flatnonzero(sizes > p)
            x = v[rows_at(p, live)]
            ok = ~np.isnan(x)
            k, x = live[ok], x[ok]
            cnt[k] += 1.0
            if compensated:
                y = x - c[k]
                t = s[k] + y
                cn = (t - s[k]) - y
                if reset:
                    cn[cn != cn] = 0.0
                c[k] = cn
                s[k] = t
            else:
                s[k] = s[k] + x
        return np.where(cnt > 0, s / np.where(cnt > 0, cnt, 1.0), np.nan)


def _sequential_max(v, rows_at, sizes):
    G = len(sizes)
    m, have = np.full(G, np.nan), np.zeros(G, dtype=bool)
    for p in range(int(sizes.max()) if G else 0):
        live = np.flatnonzero(sizes > p)
        x = v[rows_at(p, live)]
        ok = ~np.isnan(x)
        k, x = live[ok], x[ok]
        take = ~have[k] | (x > m[k])                     # strictly greater: of 0.0 and -0.0 the earlier one stays
        m[k[take]] = x[take]
        have[k] = True
    return m


def countput_twin(reps, id_min, midsum, chr_codes, compensated=True, reset=True):
    """``reps``: per replicate a mapping (DataFrame or dict) with the columns COLUMNS, in the order the rows are stacked.  Returns
    dict(baitID, otherEndID int32; Nav, Bav, score, oeID_mid float64), one entry per group in order of first appearance."""
    col = lambda name, t: np.concatenate([np.asarray(r[name], dtype=t) for r in reps]) if len(reps) else np.zeros(0, dtype=t)
    bait, oe, N = col("baitID", np.int32), col("otherEndID", np.int32), col("N", np.int32)
    Bmean, score, ds = col("Bmean", np.float64), col("score", np.float64), col("distSign", np.float64)
    midsum, chr_codes = np.asarray(midsum, dtype=np.int64), np.asarray(chr_codes, dtype=np.int32)
    rel = oe.astype(np.int64) - int(id_min)
    on_map = (rel >= 0) & (rel < len(midsum))
    on_map[on_map] = chr_codes[rel[on_map]] >= 0
    g = np.flatnonzero(~np.isnan(ds) & on_map)           # the kept rows, ascending global row index
    key = (bait[g].astype(np.int64) << 32) | (oe[g].astype(np.int64) & 0xFFFFFFFF)
    _, first, inv = np.unique(key, return_index=True, return_inverse=True)
    rank = np.empty(len(first), dtype=np.int64)
    rank[np.argsort(first)] = np.arange(len(first))      # groups numbered by first appearance
    grp = rank[inv.reshape(-1)]
    perm = np.argsort(grp, kind="stable")                # kept rows group by group, ascending g inside a group
    sizes = np.bincount(grp, minlength=len(first)).astype(np.int64)
    start = np.cumsum(sizes) - sizes
    rows_at = lambda p, live: g[perm[start[live] + p]]
    head = g[perm[start]] if len(first) else np.zeros(0, dtype=np.int64)
    return dict(baitID=bait[head], otherEndID=oe[head],
                Nav=_sequential_mean(N.astype(np.float64), rows_at, sizes, compensated, reset),
                Bav=_sequential_mean(Bmean, rows_at, sizes, compensated, reset),
                score=_sequential_max(score, rows_at, sizes),
                oeID_mid=midsum[oe[head].astype(np.int64) - int(id_min)] / 2.0)
