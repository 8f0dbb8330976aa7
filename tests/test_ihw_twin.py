"""The twin of the IHW training stage (tests/ihw_twin.py) against independent statements — the definition of the least concave majorant
in fractions.Fraction, scipy's HiGHS on the linear programme, scipy's ranks — and the library's exact knot test as compiled for the
host (chicdiff_hip_selftest_ihw_orient) against the Fraction sign.  No GPU.

Sweep against HiGHS, observed when this was written (profiles/r36_ihw_accuracy.json; ``python tests/test_ihw_twin.py`` prints them):
the twin's objective differs from the optimum by at most 1.6e-16 relative over the four cases; the bound is 1e-6 relative + 1e-6 absolute
(HiGHS's feasibility tolerance with a margin of ten)."""
import json
import math
from fractions import Fraction

import numpy as np
import pytest

import ihw_inputs as ii
import ihw_twin as tw


def training_set(k, r, f, g):
    p = k["p"] + 0.0
    return np.sort(p[(r["group"] == g + 1) & (r["fold"] != f)])


def definition_points(P):
    """Step 4's points from the definition: (0, 0), (u, #{p <= u}) per distinct u, (1, M); of equal x the largest count."""
    if len(P) == 0:
        return {Fraction(0): 0, Fraction(1): 1}
    pts = {Fraction(0): 0}
    u = np.unique(P)
    for x, c in zip(u.tolist(), np.searchsorted(P, u, side="right").tolist()):
        pts[Fraction(x)] = max(pts.get(Fraction(x), 0), c)
    pts[Fraction(1)] = max(pts.get(Fraction(1), 0), len(P))
    return pts


def majorant_failures(P, knots):
    """What the knots miss of 'vertices of the least concave majorant': returns a list of words (empty = they are it)."""
    pts = definition_points(P)
    kx = [Fraction(x) for x, _ in knots]
    kc = [int(c) for _, c in knots]
    bad = []
    if kx[0] != 0 or kx[-1] != 1 or any(a >= b for a, b in zip(kx, kx[1:])):
        return ["knots do not run from 0 to 1 ascending"]
    if any(pts.get(x) != c for x, c in zip(kx, kc)):
        bad.append("a knot is not a point")
    slopes = [Fraction(kc[j] - kc[j - 1]) / (kx[j] - kx[j - 1]) for j in range(1, len(kx))]
    if any(a <= b for a, b in zip(slopes, slopes[1:])):
        bad.append("slopes not strictly decreasing")
    xs = sorted(pts)
    j = 1
    for x in xs:
        while kx[j] < x:
            j += 1
        if kc[j - 1] + slopes[j - 1] * (x - kx[j - 1]) < pts[x]:
            bad.append("a point lies above the majorant")
            break
    return bad


@pytest.mark.parametrize("name", sorted(ii.cases()))
def test_knots_are_the_least_concave_majorant(name):
    k, r = ii.cases()[name], ii.twin(name)
    for (f, g), kn in r["knots"].items():
        assert majorant_failures(training_set(k, r, f, g), kn) == [], (name, f, g)


@pytest.mark.parametrize("name", sorted(ii.cases()))
def test_group_sizes_and_mean_weight(name):
    from scipy.stats import rankdata
    k, r = ii.cases()[name], ii.twin(name)
    kept = ~np.isnan(k["p"])
    rank = rankdata(k["cov"][kept] + 0.0, method="ordinal")
    want = np.ceil(rank / r["m"] * r["nbins"]).astype(np.int64)
    assert np.array_equal(np.bincount(want, minlength=r["nbins"] + 1), np.bincount(r["group"][kept], minlength=r["nbins"] + 1))
    assert np.array_equal(want, r["group"][kept])
    assert np.all(r["group"][~kept] == tw.NA_GROUP) and np.all(r["fold"][~kept] == -1)
    for f in range(k["nfolds"]):
        h = np.array([np.sum((r["group"] == g + 1) & (r["fold"] == f)) for g in range(r["nbins"])], dtype=np.float64)
        assert h.sum() == r["H"][f]
        if h.sum() > 0:
            assert abs(float(h @ r["weights"][:, f]) / h.sum() - 1.0) <= 1e-12, (name, f)
        else:
            assert np.all(r["weights"][:, f] == 1.0)


@pytest.mark.parametrize("seed", [11, (1 << 63) + 12345])
@pytest.mark.parametrize("nfolds", [2, 5, 16])
def test_folds_are_uniform(seed, nfolds):
    from scipy.stats import chisquare
    f = tw.folds(20011, nfolds, seed)
    assert f.min() >= 0 and f.max() < nfolds
    # six fixed draws: a uniform stream stays above 0.001 in each with probability 0.999
    assert chisquare(np.bincount(f, minlength=nfolds)).pvalue > 1e-3
    g = tw.folds(20011, nfolds, seed + 1)
    assert 0.5 / nfolds < np.mean(f == g) < 2.0 / nfolds   # another seed is another assignment


# ---- the sweep against the linear programme -----------------------------------------------------------------------------------------
def grid_case(m, nbins, frac, seed):
    p, cov = ii.signal(m, seed, frac=frac)
    return np.round(p * 1024) / 1024, cov


LP_CASES = {"m400_3bins_signal": (400, 3, 0.5, 1), "m2000_5bins_null": (2000, 5, 0.0, 2), "m6000_8bins_signal": (6000, 8, 0.3, 3),
            "m20000_10bins_null": (20000, 10, 0.0, 4)}


def fold_problem(r, p, f):
    nb = r["nbins"]
    kn = [r["knots"][(f, g)] for g in range(nb)]
    h = [int(np.sum((r["group"] == g + 1) & (r["fold"] == f))) for g in range(nb)]
    return kn, h


def F_at(K, t):
    M = float(K[-1][1])
    for j in range(1, len(K)):
        if t <= K[j][0]:
            return (K[j - 1][1] + (K[j][1] - K[j - 1][1]) * (t - K[j - 1][0]) / (K[j][0] - K[j - 1][0])) / M
    return 1.0


def lp_optimum(kn, h, alpha):
    from scipy.optimize import linprog
    nb = len(kn)
    A, b = [], []
    for g, K in enumerate(kn):
        M = float(K[-1][1])
        for j in range(1, len(K)):
            s = ((K[j][1] - K[j - 1][1]) / M) / (K[j][0] - K[j - 1][0])
            row = np.zeros(2 * nb)
            row[g], row[nb + g] = 1.0, -s                  # y_g - s t_g <= a
            A.append(row)
            b.append(K[j - 1][1] / M - s * K[j - 1][0])
    row = np.zeros(2 * nb)
    row[:nb], row[nb:] = -alpha * np.array(h, dtype=float), np.array(h, dtype=float)   # sum h t - alpha sum h y <= 0
    A.append(row)
    b.append(0.0)
    c = np.concatenate([-np.array(h, dtype=float), np.zeros(nb)])
    res = linprog(c, A_ub=np.array(A), b_ub=np.array(b), bounds=[(None, None)] * nb + [(0.0, 1.0)] * nb, method="highs")
    return res


def objective(kn, h, t):
    return float(sum(hg * F_at(K, tg) for K, hg, tg in zip(kn, h, t)))


def lp_figures(name, **wrong):
    m, nbins, frac, seed = LP_CASES[name]
    p, cov = grid_case(m, nbins, frac, seed)
    r = tw.train(p, cov, 0.05, nbins, 5, 11)
    out = []
    for f in (0, 1):
        kn, h = fold_problem(r, p, f)
        res = lp_optimum(kn, h, 0.05)
        _, _, _, t, _ = tw.sweep(kn, h, 0.05, **wrong)
        out.append(dict(fold=f, status=int(res.status), optimum=float(-res.fun), twin=objective(kn, h, t),
                        fdr_row=float(sum(hg * tg for hg, tg in zip(h, t)) - 0.05 * objective(kn, h, t))))
    return out


@pytest.mark.parametrize("name", sorted(LP_CASES))
def test_sweep_is_the_optimum_of_the_linear_programme(name):
    for fig in lp_figures(name):
        print(name, fig)
        assert fig["status"] == 0    # HiGHS alone must solve the case: a condition of the test
        assert abs(fig["twin"] - fig["optimum"]) <= 1e-6 * abs(fig["optimum"]) + 1e-6, (name, fig)
        assert fig["fdr_row"] <= 1e-9 * max(1.0, fig["optimum"])


# ---- wrong readings, each rejected on a planted case the right rule passes ----------------------------------------------------------
def test_wrong_collinear_points_kept():
    k, r = ii.cases()["grid_collinear"], ii.twin("grid_collinear")
    wrong = tw.train(k["p"], k["cov"], k["alpha"], k["nbins"], k["nfolds"], k["seed"], keep_collinear=True)
    for (f, g), kn in r["knots"].items():
        P = training_set(k, r, f, g)
        assert len(kn) == 2 and majorant_failures(P, kn) == []
        assert len(wrong["knots"][(f, g)]) == 17 and "slopes not strictly decreasing" in majorant_failures(P, wrong["knots"][(f, g)])


def test_wrong_average_ranks():
    from scipy.stats import rankdata
    k, r = ii.cases()["cov_ties"], ii.twin("cov_ties")
    want = np.ceil(rankdata(k["cov"], method="ordinal") / r["m"] * r["nbins"]).astype(np.int64)
    assert np.array_equal(r["group"], want)
    assert not np.array_equal(tw.groups(k["p"], k["cov"], k["nbins"], ties="average")[0], want)


def test_wrong_training_on_the_holdout_fold_and_h_from_training():
    k, r = ii.cases()["n1024"], ii.twin("n1024")
    args = (k["p"], k["cov"], k["alpha"], k["nbins"], k["nfolds"], k["seed"])
    holdout, htrain = tw.train(*args, train_on_holdout=True), tw.train(*args, h_from_training=True)
    assert np.all(r["T"] > 0)
    for f in range(k["nfolds"]):
        h = np.array([np.sum((r["group"] == g + 1) & (r["fold"] == f)) for g in range(r["nbins"])], dtype=np.float64)
        for g in range(r["nbins"]):
            M = int(np.sum((r["group"] == g + 1) & (r["fold"] != f)))
            assert r["knots"][(f, g)][-1][1] == M and holdout["knots"][(f, g)][-1][1] != M
        assert abs(float(h @ r["weights"][:, f]) / h.sum() - 1.0) <= 1e-12
        assert abs(float(h @ htrain["weights"][:, f]) / h.sum() - 1.0) > 1e-6


@pytest.mark.parametrize("wrong", [dict(use_F0=False), dict(descending=False)])
def test_wrong_sweeps_miss_the_optimum(wrong):
    # p on the grid with zeros among them (F(0) > 0) and signal: the right sweep is at the optimum (test above), these are not
    p, cov = grid_case(2000, 4, 0.6, 8)
    p[::7] = 0.0
    r = tw.train(p, cov, 0.05, 4, 5, 11)
    kn, h = fold_problem(r, p, 0)
    res = lp_optimum(kn, h, 0.05)
    assert res.status == 0
    right, bad = objective(kn, h, tw.sweep(kn, h, 0.05)[3]), objective(kn, h, tw.sweep(kn, h, 0.05, **wrong)[3])
    tol = 1e-6 * abs(res.fun) + 1e-6
    assert abs(right + res.fun) <= tol and abs(bad + res.fun) > 1000 * tol


def test_wrong_zero_weights_when_T_is_zero():
    k, r = ii.cases()["null_T0"], ii.twin("null_T0")
    assert np.all(r["T"] == 0.0) and np.all(r["weights"] == 1.0)
    wrong = tw.train(k["p"], k["cov"], k["alpha"], k["nbins"], k["nfolds"], k["seed"], T0_weight=0.0)
    assert np.all(wrong["weights"] == 0.0)   # mean weight 0, not 1: test_group_sizes_and_mean_weight's identity rejects it


def test_planted_sweep_ends():
    r = ii.twin("sweep_whole_segment")       # the first segment is taken whole with B + cost == 0, the second adds -0
    for f in range(3):
        kn = r["knots"][(f, 0)]
        assert [x for x, _ in kn] == [0.0, 0.25, 1.0]
        assert r["T"][f] == r["H"][f] * 0.25
    assert np.all(ii.twin("grid_collinear")["nseg"] == 1) and np.all(ii.twin("grid_one_ulp")["nseg"] == 2)
    r = ii.twin("p_zero_and_one")            # F(0) > 0 and one segment per group: the walk ends inside the first segment
    assert np.all(r["nseg"] == 3) and np.all(r["T"] > 0)


# ---- the exact knot test as compiled for the host -----------------------------------------------------------------------------------
def fraction_sign(ax, ac, bx, bc, cx, cc):
    v = (int(bc) - int(ac)) * (Fraction(cx) - Fraction(ax)) - (int(cc) - int(ac)) * (Fraction(bx) - Fraction(ax))
    return (v > 0) - (v < 0)


def planted_triples():
    t = []
    sub = 5e-324
    base = [((0.0, 0), (0.25, 1), (1.0, 4)), ((0.0, 0), (0.5, 1000), (1.0, 2000)), ((0.125, 3), (0.375, 5), (0.625, 7)),
            ((0.0, 0), (sub, 1), (2 * sub, 2)), ((0.0, 0), (3 * sub, 3), (1.0, 2 ** 31 - 1)), ((sub, 1), (2 * sub, 2), (4 * sub, 4)),
            ((0.0, 0), (1e-300, 1), (0.5, 7)), ((1e-300, 1), (0.5, 5), (1.0, 9)), ((0.0, 0), (1e-310, 1), (1e-300, 2)),
            ((0.1, 10), (0.1 + 0.2, 30), (0.7, 70)), ((1.0 / 3, 1), (2.0 / 3, 2), (1.0, 3))]
    for a, b, c in base:
        t.append((a, b, c))
        for which in range(3):
            for to in (0.0, 1.0):
                pts = [list(a), list(b), list(c)]
                pts[which][0] = float(np.nextafter(pts[which][0], to))
                if 0.0 <= pts[which][0] <= 1.0:
                    t.append(tuple(tuple(q) for q in pts))
        for dc in (-1, 1):
            if 0 <= b[1] + dc:
                t.append((a, (b[0], b[1] + dc), c))
    return t


def test_orient_host_matches_fraction_sign():
    from chicdiff_amd import hip
    rng = np.random.default_rng(17)
    n = 200000
    scale = 10.0 ** rng.choice([0, 0, -3, -8, -100, -300, -310], n)
    x = np.sort(rng.uniform(size=(n, 3)), axis=1) * scale[:, None]
    cnt = np.sort(rng.integers(0, 2 ** 31, size=(n, 3)), axis=1)
    small = rng.uniform(size=n) < 0.5
    cnt[small] = np.sort(rng.integers(0, 50, size=(int(small.sum()), 3)), axis=1)
    near = rng.uniform(size=n) < 0.6        # b on the chord as well as a double can be, then 0 or 1 ulp off
    den = np.maximum(cnt[:, 2] - cnt[:, 0], 1).astype(np.float64)
    onchord = x[:, 0] + (x[:, 2] - x[:, 0]) * ((cnt[:, 1] - cnt[:, 0]) / den)
    bx = np.where(near, onchord, x[:, 1])
    step = rng.integers(-1, 2, n)
    bx = np.where(step > 0, np.nextafter(bx, 1.0), np.where(step < 0, np.nextafter(bx, 0.0), bx))
    bx = np.clip(bx, 0.0, 1.0)
    planted = planted_triples()
    ax = np.concatenate([x[:, 0], [t[0][0] for t in planted]])
    ac = np.concatenate([cnt[:, 0], [t[0][1] for t in planted]])
    bxs = np.concatenate([bx, [t[1][0] for t in planted]])
    bc = np.concatenate([cnt[:, 1], [t[1][1] for t in planted]])
    cx = np.concatenate([x[:, 2], [t[2][0] for t in planted]])
    cc = np.concatenate([cnt[:, 2], [t[2][1] for t in planted]])
    got = hip.selftest_ihw_orient(ax, ac, bxs, bc, cx, cc)
    want = np.array([fraction_sign(*row) for row in zip(ax.tolist(), ac.tolist(), bxs.tolist(), bc.tolist(), cx.tolist(), cc.tolist())])
    assert (want == 0).sum() > 1000 and (want > 0).sum() > 1000 and (want < 0).sum() > 1000   # the set exercises all three answers
    off = np.flatnonzero(got != want)
    assert len(off) == 0, (len(off), [(ax[i], ac[i], bxs[i], bc[i], cx[i], cc[i], got[i], want[i]) for i in off[:5]])
    assert np.array_equal(np.array([tw.orient((a, b), (c, d), (e, f)) for a, b, c, d, e, f in
                                    zip(ax[-200:].tolist(), ac[-200:].tolist(), bxs[-200:].tolist(), bc[-200:].tolist(), cx[-200:].tolist(), cc[-200:].tolist())]),
                          want[-200:])


def test_pipeline_exposes_the_device_trainer():
    from chicdiff_amd import hip, pipeline
    assert callable(pipeline.ihw_device)
    caps = hip.ihw_caps()
    assert caps["max_bins"] == tw.MAX_BINS and caps["max_folds"] == tw.MAX_FOLDS and caps["auto_max_bins"] == tw.AUTO_MAX_BINS
    assert tuple(caps["chunk_lens"]) == ii.CHUNKS and len(caps["chunk_lens"]) >= 3 and min(caps["chunk_lens"]) <= 8


if __name__ == "__main__":
    figs = {name: lp_figures(name) for name in sorted(LP_CASES)}
    worst = max(abs(f["twin"] - f["optimum"]) / abs(f["optimum"]) for v in figs.values() for f in v)
    print(json.dumps(dict(bound="1e-6 relative + 1e-6 absolute", worst_relative_difference=worst, cases=figs), indent=1))
