"""getCandidateInteractions (chicdiff.R:2078-2161) restated statement by statement on Python lists and dicts — the twin the device
path (chicdiff_hip_candidate_interactions_dev, pipeline.getCandidateInteractions) is tested against.  Written independently of
the device code, the way region_universe_literal is: a stable sort by the three keys, a scan of ALL regions of the peak's bait,
math.fsum row sums.  Slow on purpose."""
import math

NA = float("nan")


def _isna(x):
    return x != x


def row_mean(values):
    """rowMeans(.SD) without na.rm: one NA makes the mean NA; the sum is exact (math.fsum), divided once."""
    if any(_isna(v) for v in values):
        return NA
    return math.fsum(values) / len(values)


def peak_delta(row, cond1, cond2, merged):
    """:2118-2127.  Returns (delta, scale): scale = max(|asinh a|, |asinh b|) is what a rounding unit of delta is measured in
    (the difference cancels); merged: |col2 - col1|, NO asinh, scale = max(|col1|, |col2|)."""
    if merged:
        a, b = row[cond1[0]], row[cond2[0]]
        return abs(b - a), max(abs(a), abs(b))
    a, b = row_mean([row[c] for c in cond1]), row_mean([row[c] for c in cond2])
    if _isna(a) or _isna(b):
        return NA, NA
    a, b = math.asinh(a), math.asinh(b)
    return abs(a - b), max(abs(a), abs(b))


def r_min(values):
    """min() without na.rm."""
    return NA if any(_isna(v) for v in values) else min(values)


def candidates_literal(bait, minOE, maxOE, p, peak_bait, peak_oe, scores, cond1, cond2, merged, score, pvcut, min_delta, margin=1e-9):
    """bait / minOE / maxOE / p: the region table's columns in its own row order; peak_bait / peak_oe / scores: the peak matrix's
    rows as read, scores[i] the list of row i's score columns; cond1 / cond2: column indices of the two conditions.

    Returns dict(selected, delta, scale, groups_all, groups): groups_all = every (baitID, oeID) group in key order as
    (peak row, min_p, delta, [region rows in key order]), groups = those the final filter keeps."""
    n, P = len(bait), len(peak_bait)
    cols = list(cond1) + list(cond2)
    # :2082-2087
    selected = [any((not _isna(scores[i][c])) and scores[i][c] > score for c in cols) for i in range(P)]
    dl = [peak_delta(scores[i], cond1, cond2, merged) for i in range(P)]
    delta, scale = [d[0] for d in dl], [d[1] for d in dl]
    for i in range(P):   # no survivor may hang on delta's last bits
        if selected[i] and not _isna(delta[i]):
            assert abs(delta[i] - min_delta) >= margin, (i, delta[i], min_delta)
    # :2098 setkey(output, baitID, minOE, maxOE) — a stable sort
    for i in range(n):
        if minOE[i] > maxOE[i]:
            raise ValueError(f"region row {i}: minOE > maxOE")
    order = sorted(range(n), key=lambda i: (bait[i], minOE[i], maxOE[i]))
    by_bait = {}
    for i in order:
        by_bait.setdefault(bait[i], []).append(i)
    # :2129 foverlaps(type = "any", mult = "all", nomatch = 0): matches in key order
    joined = []
    for i in range(P):
        if not selected[i]:
            continue
        for r in by_bait.get(peak_bait[i], []):
            if minOE[r] <= peak_oe[i] <= maxOE[r]:
                joined.append((i, r))
    # :2158-2159 setkey(outpeak, baitID, oeID); by = c("baitID", "oeID")
    joined.sort(key=lambda t: (peak_bait[t[0]], peak_oe[t[0]]))
    groups_all, seen = [], {}
    for i, r in joined:
        k = (peak_bait[i], peak_oe[i])
        if k in seen and groups_all[seen[k]][0] != i:
            raise ValueError(f"peak rows {groups_all[seen[k]][0]} and {i} share (baitID, oeID) = {k}")
        if k not in seen:
            seen[k] = len(groups_all)
            groups_all.append([i, None, delta[i], []])
        groups_all[seen[k]][3].append(r)
    for g in groups_all:
        g[1] = r_min([p[r] for r in g[3]])
    # :2161 — a NA on either side drops the row
    groups = [g for g in groups_all if (not _isna(g[1])) and (not _isna(g[2])) and g[1] <= pvcut and g[2] >= min_delta]
    return dict(selected=selected, delta=delta, scale=scale, groups_all=groups_all, groups=groups)


def candidates_brute_force(bait, minOE, maxOE, p, peak_bait, peak_oe, scores, cond1, cond2, merged, score, pvcut, min_delta):
    """Every peak against every region, O(P n), no sort of the regions: the groups the final filter keeps."""
    cols = list(cond1) + list(cond2)
    out = []
    for i in range(len(peak_bait)):
        if not any(scores[i][c] > score for c in cols):   # NaN > x is False
            continue
        rows = [r for r in range(len(bait)) if bait[r] == peak_bait[i] and minOE[r] <= peak_oe[i] and peak_oe[i] <= maxOE[r]]
        if not rows:
            continue
        rows.sort(key=lambda r: (minOE[r], maxOE[r], r))
        ps = [p[r] for r in rows]
        mp = NA if any(_isna(v) for v in ps) else min(ps)
        d = peak_delta(scores[i], cond1, cond2, merged)[0]
        if mp <= pvcut and d >= min_delta:
            out.append([i, mp, d, rows])
    out.sort(key=lambda g: (peak_bait[g[0]], peak_oe[g[0]]))
    return out


def fmt_double(x):
    """as.character(<double>): 15 significant digits (unpinned against R); NA prints as "NA"."""
    return "NA" if _isna(x) else "%.15g" % x


def candidates_table_literal(output, peaks, cond1names, cond2names, merged, score, pcol, pvcut, min_delta):
    """:2140-2161 — the final table as a list of dicts in the reference's column order.  output: dict of the results table's
    columns (lists); peaks: dict of the peak matrix's columns (lists)."""
    names = list(cond1names) + list(cond2names)
    scores = [[peaks[c][i] for c in names] for i in range(len(peaks["baitID"]))]
    c1, c2 = list(range(len(cond1names))), list(range(len(cond1names), len(names)))
    res = candidates_literal(output["baitID"], output["minOE"], output["maxOE"], output[pcol], peaks["baitID"], peaks["oeID"], scores,
                             c1, c2, merged, score, pvcut, min_delta)
    rows = []
    for i, mp, d, rs in res["groups"]:
        row = {"baitID": peaks["baitID"][i], "oeID": peaks["oeID"][i], "baitChr": peaks["baitChr"][i],
               "baitstart": output["baitstart"][rs[0]], "baitend": output["baitend"][rs[0]], "baitName": peaks["baitName"][i]}
        for c in names:
            row[c] = peaks[c][i]
        row["min_" + pcol] = mp
        row["deltaAsinhScore"] = d
        row["regionIDs"] = ",".join(str(output["regionID"][r]) for r in rs)
        row["log2FoldChanges"] = ",".join(fmt_double(output["log2FoldChange"][r]) for r in rs)
        row[pcol] = ",".join(fmt_double(output[pcol][r]) for r in rs)
        row["OEranges"] = ",".join(f"{output['OEstart'][r]}-{output['OEend'][r]}" for r in rs)
        rows.append(row)
    return rows
