"""Twin of chicdiff_hip_ihw_train_dev, written from the rule above its declaration in include/chicdiff_hip.h — not from the kernels.

    groups      stable order by covariate (-0 = +0, ties by row), group = ceil((r / m) * nbins) in double
    folds       word 0 of Philox4x32-10 at counter (i, 0, 0, STREAM), key = seed; fold = (w0 * nfolds) >> 32
    knots       least concave majorant of (0, 0), (u, #{p <= u}), (1, M) by the monotone chain; the test in exact integer arithmetic
                (a double is an integer multiple of 2^-1074)
    weights     the sweep over segments ordered by (slope descending, group, segment), every double operation in the stated order

The keyword switches of ``train`` are the WRONG readings that tests/test_ihw_twin.py plants cases against; their defaults are the rule.
"""
import math

import numpy as np

import control_twin as ct

STREAM = 16
MAX_BINS, MAX_FOLDS, AUTO_MAX_BINS = 256, 16, 40
NA_GROUP = -2 ** 31
_ONE = 1 << 1074


def exact(x):
    """x * 2^1074 as an integer (exact for every finite double)."""
    num, den = float(x).as_integer_ratio()
    return num * (_ONE // den)


def orient(a, b, c):
    """Sign of (b.c - a.c) * (c.x - a.x) - (c.c - a.c) * (b.x - a.x), exact; points are (x, count)."""
    ax = exact(a[0])
    v = (int(b[1]) - int(a[1])) * (exact(c[0]) - ax) - (int(c[1]) - int(a[1])) * (exact(b[0]) - ax)
    return (v > 0) - (v < 0)


def folds(n, nfolds, seed):
    seed = int(seed) & 0xFFFFFFFFFFFFFFFF
    i = np.arange(n, dtype=np.uint64)
    w0 = ct.philox4x32(i & np.uint64(0xFFFFFFFF), i >> np.uint64(32), 0, STREAM, seed & 0xFFFFFFFF, seed >> 32)[0]
    return ((w0 * np.uint64(nfolds)) >> np.uint64(32)).astype(np.int64)


def points(P):
    """The points of step 4 from the ascending p-values P (M = len(P)); with M = 0: (0, 0), (1, 1)."""
    M = len(P)
    if M == 0:
        return [(0.0, 0), (1.0, 1)]
    pts = []
    for k, u in enumerate(P):
        if pts and pts[-1][0] == u:
            pts[-1] = (u, k + 1)
        else:
            pts.append((u, k + 1))
    if pts[0][0] != 0.0:
        pts.insert(0, (0.0, 0))
    if pts[-1][0] != 1.0:
        pts.append((1.0, M))
    return pts


def knots(P, keep_collinear=False):
    stack = []
    for q in points(P):
        while len(stack) >= 2:
            o = orient(stack[-2], stack[-1], q)
            if o > 0 or (keep_collinear and o == 0):
                break
            stack.pop()
        stack.append(q)
    return stack


def groups(pvalue, covariate, nbins, ties="first"):
    """(group per row with NA_GROUP for left-out rows, m, nbins used)."""
    p = np.asarray(pvalue, dtype=np.float64)
    cov = np.asarray(covariate, dtype=np.float64)
    kept = ~np.isnan(p)
    bad = np.flatnonzero(kept & ~((p >= 0.0) & (p <= 1.0)))
    if len(bad):
        raise ValueError(f"pvalue[{bad[0]}] is outside [0, 1]")
    bad = np.flatnonzero(kept & np.isnan(cov))
    if len(bad):
        raise ValueError(f"covariate[{bad[0]}] is NaN on a kept row")
    m = int(kept.sum())
    if m == 0:
        raise ValueError("no kept row")
    if nbins == 0:
        nbins = max(1, min(AUTO_MAX_BINS, m // 1500))
    if not 1 <= nbins <= min(m, MAX_BINS):
        raise ValueError(f"nbins = {nbins} outside 1 .. min(m, {MAX_BINS})")
    rows = np.flatnonzero(kept)
    order = rows[np.argsort(cov[rows] + 0.0, kind="stable")]
    group = np.full(len(p), NA_GROUP, dtype=np.int64)
    if ties == "first":
        for r, i in enumerate(order, start=1):
            group[i] = math.ceil((float(r) / float(m)) * float(nbins))
    else:  # a wrong reading: average ranks
        from scipy.stats import rankdata
        rk = rankdata(cov[rows] + 0.0, method="average")
        for i, r in zip(rows, rk):
            group[i] = math.ceil((float(r) / float(m)) * float(nbins))
    return group, m, nbins


def sweep(kn, h, alpha, use_F0=True, descending=True, T0_weight=1.0):
    """Step 5 for one fold: kn[g] = knots of group g + 1, h[g] = its rows in the fold.  Returns (weights, T, H, t, number of segments)."""
    nb = len(kn)
    segs, F0 = [], []
    for g, K in enumerate(kn):
        M = float(K[-1][1])
        F0.append(float(K[0][1]) / M)
        for j in range(1, len(K)):
            d = K[j][0] - K[j - 1][0]
            dF = float(K[j][1] - K[j - 1][1]) / M
            segs.append((dF / d, g, j, d, dF))
    segs.sort(key=(lambda e: (-e[0], e[1], e[2])) if descending else (lambda e: (e[0], e[1], e[2])))
    B = 0.0
    if use_F0:
        for g in range(nb):
            B = B - (alpha * float(h[g])) * F0[g]
    t = [0.0] * nb
    for s, g, j, d, dF in segs:
        cost = float(h[g]) * (d - alpha * dF)
        if B + cost <= 0.0:
            t[g] = t[g] + d
            B = B + cost
        else:
            t[g] = t[g] + (-B / cost) * d
            break
    H = int(sum(int(x) for x in h))
    T = 0.0
    for g in range(nb):
        T = T + float(h[g]) * t[g]
    w = [T0_weight if T == 0.0 else (t[g] * float(H)) / T for g in range(nb)]
    return np.array(w), T, H, t, len(segs)


def train(pvalue, covariate, alpha, nbins, nfolds, seed, keep_collinear=False, ties="first", train_on_holdout=False, h_from_training=False,
          use_F0=True, descending=True, T0_weight=1.0):
    if not 0.0 < alpha < 1.0:
        raise ValueError(f"alpha = {alpha} outside (0, 1)")
    if not 2 <= nfolds <= MAX_FOLDS:
        raise ValueError(f"nfolds = {nfolds} outside 2 .. {MAX_FOLDS}")
    p = np.asarray(pvalue, dtype=np.float64) + 0.0
    group, m, nb = groups(p, covariate, nbins, ties=ties)
    fold = folds(len(p), nfolds, seed)
    fold[group == NA_GROUP] = -1
    kn = {}
    W = np.empty((nb, nfolds))
    T, H, nseg = [], [], []
    by_group = [np.flatnonzero(group == g + 1) for g in range(nb)]
    sorted_rows = [r[np.argsort(p[r], kind="stable")] for r in by_group]
    for f in range(nfolds):
        per_group, h = [], []
        for g in range(nb):
            r = sorted_rows[g]
            inside = fold[r] == f
            P = p[r[inside if train_on_holdout else ~inside]].tolist()
            kn[(f, g)] = knots(P, keep_collinear=keep_collinear)
            per_group.append(kn[(f, g)])
            h.append(int((~inside).sum() if h_from_training else inside.sum()))
        w, Tf, Hf, _, ns = sweep(per_group, h, alpha, use_F0=use_F0, descending=descending, T0_weight=T0_weight)
        W[:, f] = w
        T.append(Tf)
        H.append(Hf)
        nseg.append(ns)
    return dict(group=group, fold=fold, m=m, nbins=nb, knots=kn, weights=W, T=np.array(T), H=np.array(H), nseg=np.array(nseg))


def ihw_callable(seed, nbins=None, nfolds=5):
    """The twin behind pipeline.IHWcorrection's ``ihw=`` contract: (pvalue, covariate, alpha) -> (df, weights)."""
    def ihw(pvalue, covariate, alpha):
        import pandas as pd
        r = train(pvalue, covariate, alpha, 0 if nbins is None else nbins, nfolds, seed)
        g = r["group"].astype(np.float64)
        g[r["group"] == NA_GROUP] = np.nan
        return pd.DataFrame({"pvalue": np.asarray(pvalue, dtype=np.float64), "covariate": np.asarray(covariate, dtype=np.float64), "group": g}), r["weights"]
    return ihw
