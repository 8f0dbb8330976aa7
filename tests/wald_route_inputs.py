"""Whole-fit inputs for route options of the Wald stage (tests/test_wald_final_row_constant_gpu.py).

A case is a design (nA v nB), a row count, a value of "line_search_spread" and, for the small fits, a given trend (no trend fit, no
simulation: the Wald stage is what is under test).  Rows come from synth.make; planted from row 8 on where the matrix has 63 rows or more:
  floor   group A = (0, .., 0, 1), group B ordinary counts: group A's start value puts nf * e^eta below minmu = 0.5;
  huge    one count of 10^6 among zeros: the first IRLS solve leaves |beta| far beyond 30, the row goes to the optim fallback;
  huge2   one count of 10^6 beside ordinary counts (the same end by another way in);
  zero    all-zero rows;
  big     one count of 4 000 * 2^t, t = 0 .. 5, beside ordinary counts: the first solve stays inside 30 and the IRLS gives up later.
first_step() is a NumPy restatement of the IRLS's first solve from the least-squares start, for the asserts on what a matrix holds.
"""
import numpy as np

from chicdiff_amd import synth

THETA = 0.5
GIVEN_TREND = dict(trendCoef=(0.05, 2.0), dispPriorVar=1.0)
MINMU = 0.5

# name -> (nA, nB, n, line_search_spread values, trend given)
SHAPES = {
    "4v4-n1": (4, 4, 1, (0, 1), True),
    "4v4-n63": (4, 4, 63, (0, 1), True),
    "4v4-n65": (4, 4, 65, (0, 1), True),
    "4v4-n4097": (4, 4, 4097, (0, 1), False),
    "1v1-n4097": (1, 1, 4097, (0, 1), True),  # S = p: the library refuses the fit (no residual degrees of freedom), on every route alike
    "1v2-n4097": (1, 2, 4097, (0, 1), True),  # ... so the smallest design that is fitted stands beside it
    "3v5-n4097": (3, 5, 4097, (0, 1), False),
    "8v8-n4097": (8, 8, 4097, (0, 1), False),
    "2v2-n140000": (2, 2, 140_000, (1,), False),  # above 131 072 rows: the IRLS runs in its schedule's order (4097 rows: natural order)
}
CASES = [(name, spread) for name, s in SHAPES.items() for spread in s[3]]
_cache = {}


def make_shape(name):
    if name in _cache:
        return _cache[name]
    nA, nB, n, _, given = SHAPES[name]
    S = nA + nB
    group = np.array([0] * nA + [1] * nB, dtype=np.int32)
    d = synth.make(n, S)
    counts, nf, mu = d["counts"].copy(), d["nf"], d["mu"]
    planted = {}
    if n == 1:
        counts = np.maximum(counts, 1)  # the size factors need a row without a zero
    if n >= 63:
        A, B = np.flatnonzero(group == 0), np.flatnonzero(group == 1)
        rows = np.arange(8, 14)
        for t, i in enumerate(rows):
            counts[i, A] = 0
            counts[i, A[-1]] = 1
            counts[i, B] = 30 + 7 * t + np.arange(len(B))
        planted["floor"] = rows
        rows = np.arange(14, 18)
        for t, i in enumerate(rows):
            counts[i] = 0
            counts[i, (t * 3) % S] = 10 ** 6
        planted["huge"] = rows
        rows = np.arange(18, 22)
        for t, i in enumerate(rows):
            counts[i] = np.maximum(counts[i], 1)
            counts[i, (t * 5 + 1) % S] = 10 ** 6
        planted["huge2"] = rows
        rows = np.array([22, 23, n // 2, n - 1])
        counts[rows] = 0
        planted["zero"] = rows
        rows = np.arange(24, 30)
        for t, i in enumerate(rows):
            counts[i] = np.maximum(counts[i], 1)
            counts[i, (t * 3 + 2) % S] = 4000 * 2 ** t
        planted["big"] = rows
    case = dict(name=name, n=n, S=S, group=group, counts=np.ascontiguousarray(counts, dtype=np.int32),
                fullmean=np.ascontiguousarray(nf * (mu[:, None] / S)), planted=planted, opts=dict(GIVEN_TREND) if given else None)
    _cache[name] = case
    return case


def first_step(counts, nf, group, alpha):
    """-> (a sample of the row is floored at minmu at the least-squares start, beta0, beta1 after the first solve); natural-log scale"""
    y = counts.astype(np.float64)
    B = (np.asarray(group) == 1)[None, :]
    A = ~B
    nA, nB = int(A.sum()), int(B.sum())
    l = np.log(y / nf + 0.1)
    lA, lB = (l * A).sum(1) / nA, (l * B).sum(1) / nB
    eta = np.where(B, lB[:, None], lA[:, None])
    raw = nf * np.exp(eta)
    floored = raw < MINMU
    m = np.where(floored, MINMU, raw)
    w = m / (1.0 + alpha[:, None] * m)
    z = np.where(floored, np.log(MINMU) - np.log(nf), eta) + (y - m) / m
    lam = 1e-6 / np.log(2.0) ** 2
    wA, wB, zA, zB = (w * A).sum(1), (w * B).sum(1), (w * z * A).sum(1), (w * z * B).sum(1)
    m00, m01, m11 = wA + wB + lam, wB, wB + lam
    det = m00 * m11 - m01 * m01
    return floored.any(1), (m11 * (zA + zB) - m01 * zB) / det, (m00 * zB - m01 * (zA + zB)) / det


def oracle_view(case):
    """What the CPU oracle makes of the case: its own size factors and offsets, its fit, and first_step at its dispersions."""
    if "oracle" in case:
        return case["oracle"]
    from oracle import oracle
    sf = oracle.size_factors(case["counts"])
    nf = oracle.offsets(case["fullmean"], sf, THETA)
    ref = oracle.nbglm_fit(case["counts"], nf, case["group"], **(case["opts"] or {}))
    live = ref["allZero"] == 0
    with np.errstate(all="ignore"):
        fl, b0, b1 = first_step(case["counts"], nf, case["group"], np.where(live, ref["dispersion"], 1.0))
    case["oracle"] = dict(nf=nf, ref=ref, live=live, floored=fl & live, beyond30=live & ((np.abs(b0) > 30) | (np.abs(b1) > 30)))
    return case["oracle"]


ALL_COLUMNS = ["baseMean", "baseVar", "dispGeneEst", "dispFit", "dispMAP", "dispersion", "log2FoldChange", "lfcSE", "stat", "pvalue",
               "intercept", "interceptSE", "deviance", "maxCooks", "dispGeneIter", "dispIter", "dispOutlier", "betaConv", "betaIter",
               "allZero", "cooksArgmax"]


def fit(ctx, case, spread):
    """One whole fit -> ("ok", columns as host arrays, scalars) or ("error", message)"""
    from chicdiff_amd import hip
    ctx.set_option("line_search_spread", spread)
    try:
        dk = ctx.to_device(case["counts"], np.int32)
        dfm = ctx.to_device(case["fullmean"], np.float64)
        opts = hip.default_opts(**case["opts"]) if case["opts"] else None
        try:
            out, sc = ctx.wald_test(dk, dfm, case["group"], theta=THETA, want=ALL_COLUMNS, opts=opts)
        except hip.ChicdiffHipError as e:
            return "error", str(e), None
        return "ok", {k: v.cpu().numpy() for k, v in out.items()}, sc
    finally:
        ctx.set_option("line_search_spread", 1)


def same_scalars(a, b, but=()):
    assert a.keys() == b.keys()
    for k in a:
        if k not in but:
            assert np.array_equal(np.asarray(a[k]), np.asarray(b[k]), equal_nan=True), (k, a[k], b[k])
