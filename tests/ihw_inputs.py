"""Inputs of the IHW training tests (tests/test_ihw_twin.py, tests/test_ihw_gpu.py): name -> dict(p, cov, nbins, nfolds, seed, alpha).

The cases are small on purpose: the chunk lengths of the library start at 4, so chunk and group edges are planted in a few hundred rows.
"""
import functools

import numpy as np

import ihw_twin as tw

CHUNKS = (4, 32, 128)   # what chicdiff_hip_ihw_caps reports (tests/test_ihw_gpu.py checks that it still does)


def signal(n, seed, frac=0.3, quant=None):
    """p-values whose signal density falls with the covariate; covariate = a positive 'distance'."""
    rng = np.random.default_rng(seed)
    cov = np.exp(rng.uniform(0.0, 10.0, n))
    alt = rng.uniform(size=n) < frac * np.exp(-np.log(cov) / 3.0)
    p = np.where(alt, rng.beta(0.05, 4.0, n), rng.uniform(size=n))
    if quant:
        p = np.round(p * quant) / quant
    return p, cov


def by_fold_class(n, nfolds, seed, pattern):
    """Every fold class gets whole copies of ``pattern`` (the rows left over get NaN): the training set of every fold is then a whole
    number of copies too."""
    f = tw.folds(n, nfolds, seed)
    p = np.full(n, np.nan)
    for k in range(nfolds):
        rows = np.flatnonzero(f == k)
        rows = rows[: len(rows) // len(pattern) * len(pattern)]
        p[rows] = np.resize(np.asarray(pattern, dtype=np.float64), len(rows))
    return p


def _case(p, cov, nbins, nfolds=5, seed=11, alpha=0.05):
    return dict(p=np.asarray(p, dtype=np.float64), cov=np.asarray(cov, dtype=np.float64), nbins=nbins, nfolds=nfolds, seed=seed, alpha=alpha)


def _build():
    c = {}
    rng = np.random.default_rng(5)
    for m in (1, 2, 3):
        c[f"m{m}_one_bin"] = _case(rng.uniform(size=m), rng.uniform(size=m), 1, nfolds=2)
    c["m3_bins_eq_m"] = _case([0.2, 0.01, 0.7], [3.0, 1.0, 2.0], 3, nfolds=2)
    c["m7_bins_eq_m"] = _case(rng.uniform(size=7), rng.uniform(size=7), 7, nfolds=3)
    for m in (1499, 1500, 3000):
        p, cov = signal(m, m)
        c[f"auto_m{m}"] = _case(p, cov, 0)
    for n in (255, 256, 257, 1023, 1024, 1025):
        p, cov = signal(n, n)
        c[f"n{n}"] = _case(p, cov, 3)
    p, cov = signal(257, 1)
    c["n257_one_bin"] = _case(p, cov, 1)
    p, cov = signal(20011, 3)
    c["n20011"] = _case(p, cov, 10)
    c["n20011_seed2"] = _case(p, cov, 10, seed=(1 << 63) + 12345)
    for L in CHUNKS:   # two groups of exactly s rows each
        for s in (L - 1, L, L + 1, 2 * L + 1):
            p, cov = signal(2 * s, 100 + s)
            c[f"group_size_{s}"] = _case(p, cov, 2, nfolds=3)
    p, cov = signal(300, 7, quant=8)   # nine distinct p-values: runs of equal p across every chunk and group edge
    c["p_runs"] = _case(p, cov, 3)
    for name, v in (("all_p_equal", 0.3), ("all_p_zero", 0.0), ("all_p_one", 1.0)):
        c[name] = _case(np.full(200, v), rng.uniform(size=200), 3)
    c["p_zero_and_one"] = _case(np.where(rng.uniform(size=200) < 0.4, 0.0, 1.0), rng.uniform(size=200), 3)
    c["p_minus_zero"] = _case(np.where(rng.uniform(size=64) < 0.5, -0.0, rng.uniform(size=64)), rng.uniform(size=64), 2)
    grid = np.arange(1, 17) / 16.0   # equal counts on a grid that ends at 1: every inner point lies on the chord from (0, 0) to (1, M)
    c["grid_collinear"] = _case(by_fold_class(700, 3, 11, grid), rng.uniform(size=700), 1, nfolds=3)
    up = by_fold_class(700, 3, 11, grid)
    up[up == 0.5] = np.nextafter(0.5, 0.0)   # the point (0.5, M / 2) one ulp to the left: now strictly above the chord, a knot
    c["grid_one_ulp"] = _case(up, c["grid_collinear"]["cov"], 1, nfolds=3)
    tiny = np.array([5e-324, 1e-323, 2.0 ** -1060, 2.2250738585072014e-308, 1e-300, 1e-310, 0.0, 0.5, 1.0])
    c["subnormal_p"] = _case(rng.choice(tiny, 150), rng.uniform(size=150), 2, nfolds=3)
    p, cov = signal(600, 9)
    q = p.copy()
    q[rng.uniform(size=600) < 0.2] = np.nan
    c["nan_scattered"] = _case(q, cov, 3)
    q = p.copy()
    q[:130] = np.nan
    q[300:428] = np.nan
    covn = cov.copy()
    covn[:130] = np.nan   # a left-out row's covariate is never read
    c["nan_blocks"] = _case(q, covn, 3)
    p, cov = signal(240, 13)
    c["cov_ties"] = _case(p, np.floor(np.log(cov)), 4)          # eleven covariate values: ties across every group edge
    cz = rng.choice(np.array([-0.0, 0.0, 1.0, np.inf]), 240)
    c["cov_zeros_inf"] = _case(p, cz, 3)
    c["m8_folds16"] = _case(rng.uniform(size=8), rng.uniform(size=8), 8, nfolds=16)   # empty training sets and empty hold-out folds
    c["null_T0"] = _case(rng.uniform(0.2, 1.0, 400), rng.uniform(size=400), 4)         # no slope reaches 1 / alpha: T = 0, weights 1
    # every training set is two copies of (0, 0, .25, .25, 1, 1, 1, 1) x 2: B + cost of the first segment is exactly 0 at alpha = 0.5
    c["sweep_whole_segment"] = _case(by_fold_class(200, 3, 11, [0, 0, 0.25, 0.25, 1, 1, 1, 1]), rng.uniform(size=200), 1, nfolds=3, alpha=0.5)
    p, cov = signal(500, 21, frac=0.9)
    c["sweep_inside_first"] = _case(np.minimum(p, 0.999) * 0.5 + 0.25, cov, 2)
    return c


@functools.lru_cache(maxsize=None)
def cases():
    return _build()


@functools.lru_cache(maxsize=None)
def twin(name):
    """The twin's result of a case, computed once and shared (never modified by a test)."""
    k = cases()[name]
    return tw.train(k["p"], k["cov"], k["alpha"], k["nbins"], k["nfolds"], k["seed"])
