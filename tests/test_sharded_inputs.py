"""The inputs of the small sharded suite (tests/sharded_inputs.py) are what their names say — checked on the CPU with the project's
oracle (oracle.nbglm_fit on the offsets of the fused call: size factors, theta = 0.5) and tests/norm_twin.py, so that a GPU case that
passes has passed on the edge it was built for:

  every case      the single-rank parametric trend converges (no local substitute, no failure) and dispPriorVar is finite; the splits
                  add up; every split, design and variant of the issue's list occurs
  zero_shard      the planted rank's rows are all zero
  no_ratio_shard  the planted rank has no all-positive row (and no all-zero one: its rows are fitted)
  flat_shard      the planted rank's gene-wise estimates are below 10 minDisp (none usable for the trend)
  ties            per column, the index (both indices, when the count is even) of the size-factor median lies strictly inside the run of
                  keys equal to the copied row's; the run has members on at least two ranks; the twin's size factor is exp(that key).
                  The median of the trend's residuals is the copies' residual as well
"""
import numpy as np
import pytest

import norm_twin
import sharded_inputs as si

ST_TREND_FAILED, ST_PRIORVAR_MC, ST_TREND_LOCAL = 1, 2, 16


@pytest.fixture(scope="module")
def oracle():
    from oracle import oracle as o
    o.build()
    return o


_fits = {}


def oracle_fit(oracle, case, zero_rows=True):
    key = (case, zero_rows)
    if key not in _fits:
        inp = si.build(case, zero_rows=zero_rows)
        sf = oracle.size_factors(inp["counts"])
        nf = oracle.offsets(inp["fm"], sf, 0.5)
        _fits[key] = (sf, oracle.nbglm_fit(inp["counts"], nf, inp["group"]))
    return _fits[key]


def test_the_issues_lists_are_covered():
    assert {c[0] for c in si.CASES} == set(si.SPLITS) == {"w2", "w3", "w4", "w5", "w7", "w8"}
    assert {c[1] for c in si.CASES} == set(si.DESIGNS)
    assert {c[2] for c in si.CASES} == {"base", "zero_shard", "no_ratio_shard", "flat_shard", "ties"}
    assert si.SPLITS["w8"] == [513] * 5 + [512] * 3
    assert ("w7", "S5", "base", None) in si.UNEQUAL and all(c in si.CASES for c in si.UNEQUAL)
    assert {si.DESIGNS[c[1]][0] for c in si.GRID_CASES} == {4, 8}
    for split, rows in si.SPLITS.items():
        b = si.bounds(split)
        assert [hi - lo for lo, hi in b] == rows and b[0][0] == 0 and all(b[r][1] == b[r + 1][0] for r in range(len(b) - 1))
        assert b[-1][1] <= 5000


@pytest.mark.parametrize("case,zero_rows", [(c, True) for c in si.CASES] + [(c, False) for c in si.GRID_CASES],
                         ids=[si.case_id(c) for c in si.CASES] + [si.case_id(c) + "-grid" for c in si.GRID_CASES])
def test_single_rank_parametric_trend_converges(oracle, case, zero_rows):
    inp = si.build(case, zero_rows=zero_rows)
    sf, fit = oracle_fit(oracle, case, zero_rows)
    S, p = inp["S"], 2 if inp["group"].any() else 1
    assert np.all(np.isfinite(sf)) and np.all(sf > 0)
    assert not (fit["status"] & (ST_TREND_FAILED | ST_TREND_LOCAL)), fit["status"]
    assert np.all(np.isfinite(fit["trendCoef"])) and np.isfinite(fit["dispPriorVar"])
    assert bool(fit["status"] & ST_PRIORVAR_MC) == (S - p <= 3)
    assert bool((inp["counts"].sum(axis=1) == 0).any()) == zero_rows
    if not zero_rows:   # the theta grid's fit: design ~1, every total deviance finite
        fit1 = oracle.nbglm_fit(inp["counts"], oracle.offsets(inp["fm"], sf, 0.5), np.zeros(S, dtype=np.int32))
        assert not (fit1["status"] & (ST_TREND_FAILED | ST_TREND_LOCAL)) and np.isfinite(fit1["sumDeviance"])


def planted(variant):
    return [c for c in si.CASES if c[2] == variant]


@pytest.mark.parametrize("case", planted("zero_shard"), ids=si.case_id)
def test_zero_shard_is_all_zero(case):
    inp = si.build(case)
    lo, hi = inp["bounds"][case[3]]
    assert 0 < case[3] < len(inp["bounds"]) - 1 and hi > lo      # a middle rank
    assert not inp["counts"][lo:hi].any()
    assert all((inp["counts"][a:b] > 0).all(axis=1).any() for r, (a, b) in enumerate(inp["bounds"]) if r != case[3] and b - a > 1)


@pytest.mark.parametrize("case", planted("no_ratio_shard"), ids=si.case_id)
def test_no_ratio_shard_has_no_all_positive_row(case):
    inp = si.build(case)
    lo, hi = inp["bounds"][case[3]]
    k = inp["counts"][lo:hi]
    assert not (k > 0).all(axis=1).any()
    assert (k.sum(axis=1) > 0).all()     # ... but every row is fitted


@pytest.mark.parametrize("case", planted("flat_shard"), ids=si.case_id)
def test_flat_shard_sits_at_the_floor(oracle, case):
    inp = si.build(case)
    lo, hi = inp["bounds"][case[3]]
    _, fit = oracle_fit(oracle, case)
    g = fit["dispGeneEst"][lo:hi]
    print("flat shard: largest gene-wise estimate", g.max(), "of", hi - lo, "rows")
    assert np.all(g < 10 * si.MIN_DISP), g.max()
    assert (inp["counts"][lo:hi] > 0).all()      # (they do give size-factor ratios: on the medians)


@pytest.mark.parametrize("case", planted("ties"), ids=si.case_id)
def test_ties_hold_both_medians(oracle, case):
    inp = si.build(case)
    counts, rows = inp["counts"], inp["tie_rows"]
    row_k, _ = inp["tie_source"]
    is_copy = (counts == row_k[None, :]).all(axis=1)
    assert is_copy[rows].all()
    on_ranks = [int(is_copy[lo:hi].sum()) for lo, hi in inp["bounds"]]
    assert sum(c > 0 for c in on_ranks) >= 2 and all(c > 0 for c in on_ranks), on_ranks
    usable = (counts > 0).all(axis=1)
    m, copies = int(usable.sum()), int(is_copy.sum())
    assert (row_k > 0).all() and 2 * copies > m
    lg = np.log(counts[usable].astype(np.float64))
    keys = lg - lg.mean(axis=1, keepdims=True)
    tie_key = np.log(row_k.astype(np.float64)) - np.log(row_k.astype(np.float64)).mean()
    sf, unit, used = norm_twin.size_factors(counts)
    assert used == m
    lo_idx, hi_idx = ((m // 2, m // 2) if m % 2 else (m // 2 - 1, m // 2))
    for j in range(inp["S"]):
        below, above = int((keys[:, j] < tie_key[j] - 1e-9).sum()), int((keys[:, j] > tie_key[j] + 1e-9).sum())
        assert below + above + copies == m, (j, below, above, copies, m)    # nothing else within 1e-9 of the run: the run is the copies
        first, last = below, below + copies - 1
        assert first < lo_idx and hi_idx < last, (j, first, lo_idx, hi_idx, last)
        assert abs(float(sf[j]) - np.exp(tie_key[j])) <= 1e-12 * float(sf[j])
    # the median of the residuals log(dispGeneEst) - log(dispFit) over the rows the MAD takes (estimate >= 100 minDisp): a copy's too
    _, fit = oracle_fit(oracle, case)
    g, f = fit["dispGeneEst"], fit["dispFit"]
    take = (fit["allZero"] == 0) & (g >= 100 * si.MIN_DISP)
    res = np.log(g[take]) - np.log(f[take])
    tie_res = np.log(g[rows[0]]) - np.log(f[rows[0]])
    assert take[rows].all() and np.all(res[is_copy[take]] == tie_res)
    nb, na, mm = int((res < tie_res).sum()), int((res > tie_res).sum()), len(res)
    assert nb < (mm - 1) // 2 and na < (mm - 1) // 2, (nb, na, mm)
