"""The inputs of tests/theta_inputs.py hold what they say, and the yardstick of tests/test_gpu_theta_scan.py stands on its own: on every
trend-edges case the 50-digit twin (tests/disp_twin.global_stage) converges with no decision nearer than 1e-9 to its threshold (so
test_disp_twin.judge_global excuses nothing there), the oracle's routines pass that judge without violation, the tiled column has the
base case's median and MAD by bits, and the oracle's deviance totals of every scan are at least 1e-6 apart (relative) at the minimum —
ten times the 1e-7 the device is held to per theta, which makes "the same argmin" a fair requirement.  No GPU.

The helpers the GPU tests share are here too: the oracle's routines on a set of stage columns (`yardstick`), the judge of a stage
case (`judge_stage`), the rule and the row formula of the residual column (`judge_resid`)."""
import time

import mpmath as mp
import numpy as np
import pytest

import disp_twin as dt
import test_disp_twin as td
import theta_inputs as th
import trend_inputs as ti

NEAR_MIN = 1e-9   # judge_global excuses a decision only within this distance of its threshold
GAP_MIN = 1e-6    # relative gap between the two smallest deviance totals of a scan
STAGE_CASES = [n for n in th.EDGES if n != "trend-edges-tiled"]


@pytest.fixture(scope="module")
def oracle():
    from oracle import oracle as o
    o.build()
    return o


def fit_of(case):
    """What judge_global reads of a fit: S, and a group that says p."""
    g = np.zeros(case["S"], dtype=np.int32)
    if case["p"] == 2:
        g[case["S"] // 2:] = 1
    return dict(S=case["S"], group=g)


_TWINS = {}


def twin_of(name):
    """dt.global_stage on a trend-edges case (the tiled case: on its 599 rows), once per session."""
    base = th.edge_case(name).get("base", name)
    if base not in _TWINS:
        c = th.edge_case(base)
        with mp.workdps(dt.DPS):
            _TWINS[base] = dt.global_stage(c["baseMean"], c["dispGeneEst"], c["S"], c["p"])
    return _TWINS[base]


def yardstick(oracle, baseMean, dispGeneEst, allZero, S, p):
    """The oracle's routines on stage columns, as tests/test_gpu_disp.py::test_global_stage_against_twin uses them: (dispFit column, scalars,
    residual column)."""
    bm, al = np.asarray(baseMean, dtype=np.float64), np.asarray(dispGeneEst, dtype=np.float64)
    nz = np.asarray(allZero) == 0
    with np.errstate(invalid="ignore", divide="ignore"):
        use = nz & (al > ti.T100)
        keep = nz & (al >= ti.T100)
        coefs, it, rc = oracle.parametric_dispersion_fit(bm[use], al[use])
        assert rc == 0, rc
        fitted = coefs[0] + coefs[1] / bm
        resid = np.where(keep, np.log(al) - np.log(fitted), np.nan)
    x = np.ascontiguousarray(resid[keep])
    dev_abs = np.ascontiguousarray(np.abs(x - oracle.lib().oracle_median(oracle._pd(x.copy()), len(x))))
    v = (1.4826 * oracle.lib().oracle_median(oracle._pd(dev_abs), len(x))) ** 2
    m = S - p
    sc = dict(trendCoef=coefs, trendOuterIter=it, varLogDispEsts=v,
              dispPriorVar=max(v - oracle.lib().oracle_trigamma(m / 2.0), 0.25) if m > 3 else oracle.prior_var_mc(x, m))
    return fitted, sc, resid


def judge_resid(baseMean, dispGeneEst, allZero, coefs, resid, rows=None):
    """The residual column of the global stage on REPORTED coefficients.  The rule of resid_kernel: an all-zero row or dispGeneEst below
    100 minDisp gives NaN, every other row log(dispGeneEst) - log(c0 + c1 / baseMean), finite.  Returns (rows whose NaN pattern is wrong,
    worst error of a finite residual in units U (|log a| + |log f|) + U (|c0| + |c1 / m|) / f — the two logarithms and the fitted value
    rounded once each)."""
    bm, al, az = np.asarray(baseMean), np.asarray(dispGeneEst), np.asarray(allZero)
    rows = range(len(bm)) if rows is None else rows
    wrong, worst = [], 0.0
    with mp.workdps(dt.DPS):
        c0, c1 = (mp.mpf(float(v)) for v in coefs)
        for i in rows:
            want_nan = bool(az[i]) or not al[i] >= ti.T100
            if want_nan != bool(np.isnan(resid[i])) or (not want_nan and not np.isfinite(resid[i])):
                wrong.append(int(i))
                continue
            if want_nan:
                continue
            a, f = mp.mpf(float(al[i])), c0 + c1 / mp.mpf(float(bm[i]))
            unit = dt.U * (abs(mp.log(a)) + abs(mp.log(f))) + dt.U * (abs(c0) + abs(c1 / mp.mpf(float(bm[i])))) / f
            worst = max(worst, float(abs(mp.mpf(float(resid[i])) - (mp.log(a) - mp.log(f))) / unit))
    return wrong, worst


def judge_stage(case, scalars, dispFit=None, fit_rows=()):
    """judge_global on a trend-edges case (the tiled case: against the twin of its 599 rows; `dispFit`, where the route writes the column,
    judged on `fit_rows`)."""
    base = th.edge_case(case.get("base", case["name"]))
    cols = dict(baseMean=base["baseMean"], dispGeneEst=base["dispGeneEst"], dispFit=dispFit if dispFit is not None else np.full(len(base["baseMean"]), np.nan))
    return td.judge_global(fit_of(case), cols, scalars, twin=twin_of(case["name"]), fit_rows=list(fit_rows))


_DEV = {}


def oracle_deviances(oracle, name):
    """The oracle's deviance total of every theta of a scan case (design ~1), once per session."""
    if name not in _DEV:
        c = th.scan_case(name)
        g0 = np.zeros(c["counts"].shape[1], dtype=np.int32)
        _DEV[name] = np.array([oracle.nbglm_fit(c["counts"], oracle.offsets(c["FullMean"], c["sf"], t), g0)["sumDeviance"] for t in c["thetas"]])
    return _DEV[name]


# ---------------------------------------------------------------------------------------------------------------------------
def test_scan_cases_hold_what_they_say(oracle):
    for name, (n, S) in th.SCANS.items():
        c = th.scan_case(name)
        k = c["counts"]
        assert k.dtype == np.int32 and k.shape[1] == S and n - 20 <= len(k) <= n and c["FullMean"].shape == k.shape, (name, k.shape)
        F = c["FullMean"]  # (synth.make plants NA in one cell of 1 % of the rows on its own)
        assert (k.sum(1) > 0).all() and k.min() >= 0 and not np.isinf(F).any() and (F[~np.isnan(F)] > 0).all() and np.isnan(F).sum() < 0.02 * len(F)
        assert np.array_equal(c["sf"], oracle.size_factors(k)) and c["thetas"] == [0.0, 0.25, 0.5, 0.75, 1.0]
    base = th.scan_case("scan-S8")
    n, S = base["counts"].shape
    z = th.scan_case("scan-zero")
    rows = z["planted"]["zero"]
    assert list(rows) == [0, n // 2, n - 1] and np.array_equal(np.flatnonzero(z["counts"].sum(1) == 0), rows)
    live = np.setdiff1d(np.arange(n), rows)
    assert np.array_equal(z["counts"][live], base["counts"][live]) and np.array_equal(z["FullMean"], base["FullMean"], equal_nan=True)
    assert np.array_equal(z["sf"], oracle.size_factors(z["counts"]))
    na = th.scan_case("scan-na")
    places = na["planted"]["na"]
    assert [i for i, _ in places] == [0, n - 1, (n // 256) * 256] and 0 < places[2][0] < n - 1 and n % 256
    assert not any(np.isnan(base["FullMean"][i, j]) for i, j in places)
    holes = set(map(tuple, np.argwhere(np.isnan(na["FullMean"])))) - set(map(tuple, np.argwhere(np.isnan(base["FullMean"]))))
    assert sorted(holes) == sorted(places)
    mask = ~np.isnan(na["FullMean"])
    assert np.array_equal(na["FullMean"][mask], base["FullMean"][mask]) and np.array_equal(na["counts"], base["counts"])
    assert th.SUM_SIZES == (1, 255, 256, 257, 1025)
    for m in th.SUM_SIZES:
        s = th.sum_case(m)
        assert s["counts"].shape == (m, S) and np.array_equal(s["counts"], base["counts"][:m]) and (s["counts"].sum(1) > 0).all()
        assert s["opts"] == dict(trendCoef=(0.05, 2.0), dispPriorVar=1.0)


@pytest.mark.parametrize("name", list(th.SCANS) + ["scan-na"])
def test_scan_deviance_gap(oracle, name):
    """The two smallest of the oracle's totals are at least 1e-6 apart, relative: the device, held to 1e-7 of each, has the same argmin."""
    dev = oracle_deviances(oracle, name)
    s = np.sort(dev)
    gap = (s[1] - s[0]) / abs(s[0])
    print(name, dev, f"gap {gap:.3g}")
    assert np.isfinite(dev).all() and gap >= GAP_MIN, (name, dev, gap)


def test_scan_zero_total_is_na(oracle):
    """sum() without na.rm: the oracle's totals of scan-zero are all NaN."""
    assert np.isnan(oracle_deviances(oracle, "scan-zero")).all()


def test_trend_edges_planted_rows():
    """The columns of every trend-edges case: NaN on the all-zero rows alone; the rows at, below and above 100 minDisp; and — in 50 digits,
    with the start coefficients (0.1, 1) — the first round's filter drops exactly the planted out-of-range rows (and the rows just above
    100 minDisp, whose ratio is 1e-5 at most) and keeps their in-range neighbours, all eight at relative distance 1e-6 from a bound."""
    for name in STAGE_CASES:
        c = th.edge_case(name)
        p, n = c["planted"], len(c["baseMean"])
        bm, al = c["baseMean"], c["dispGeneEst"]
        assert n == (599 if name.endswith("599") else int(name.rsplit("-", 1)[1])) and c["opts"] == dict(fitType=0) and c["p"] == 1
        assert np.array_equal(np.flatnonzero(np.isnan(bm)), p["zero"]) and np.array_equal(np.flatnonzero(np.isnan(al)), p["zero"])
        assert np.array_equal(np.flatnonzero(c["allZero"]), p["zero"]) and p["zero"][0] == 0 and p["zero"][-1] == n - 1
        assert (al[p["below"]] < ti.T100).all() and (al[p["at"]] == ti.T100).all() and (al[p["above"]] == np.nextafter(ti.T100, 1.0)).all()
        live = np.setdiff1d(np.arange(n), np.concatenate([p["zero"], p["below"], p["at"]]))
        assert (al[live] > ti.T100).all()
        with mp.workdps(dt.DPS):
            ratio = {int(i): mp.mpf(float(al[i])) / (mp.mpf(0.1) + 1 / mp.mpf(float(bm[i]))) for i in live}
            out = sorted(i for i, r in ratio.items() if not mp.mpf(1e-4) < r < mp.mpf(15))
            if name.endswith("599"):
                assert len(p["zero"]) == 72 and np.array_equal(p["zero"][1:-1], np.arange(260, 330))
                assert out == sorted(list(p["out"]) + list(p["above"])), (out, p["out"])
                dist = {i: float(min(abs(ratio[i] / mp.mpf(1e-4) - 1), abs(ratio[i] / mp.mpf(15) - 1))) for i in list(p["out"]) + list(p["inside"])}
                assert all(abs(d / 1e-6 - 1) < 1e-6 for d in dist.values()), dist
                assert sum(ratio[int(i)] < 1 for i in p["out"]) == 2 and sum(ratio[int(i)] < 1 for i in p["inside"]) == 2
            else:
                assert out == []
    t = th.edge_case("trend-edges-tiled")
    b = th.edge_case("trend-edges-599")
    assert len(t["baseMean"]) == 599 * 439 == 262961 > 2 * 512 * 256
    for k in ("baseMean", "dispGeneEst", "allZero"):
        assert np.array_equal(t[k].reshape(439, 599), np.broadcast_to(b[k], (439, 599)), equal_nan=True)


@pytest.mark.parametrize("name", STAGE_CASES)
def test_trend_edges_twin_and_yardstick(oracle, name):
    """The twin converges, no decision of it lies within 1e-9 of its threshold, and the oracle's routines pass judge_global on the case:
    no violation, nothing excused, every error below the separation."""
    c = th.edge_case(name)
    t0 = time.perf_counter()
    gs = twin_of(name)
    assert not gs["failed"] and gs["rounds"] >= 2
    assert gs["near"] >= NEAR_MIN, float(gs["near"])
    fitted, sc, resid = yardstick(oracle, c["baseMean"], c["dispGeneEst"], c["allZero"], c["S"], c["p"])
    res = judge_stage(c, sc, fitted, range(len(fitted)))
    wrong, worst = judge_resid(c["baseMean"], c["dispGeneEst"], c["allZero"], sc["trendCoef"], resid)
    print(f"{name}: {time.perf_counter() - t0:.1f} s; rounds {gs['rounds']}, closest decision {float(gs['near']):.3g}; {res['errors']}; resid {worst:.3g}")
    assert not res["violations"] and res["near"] == 0, res["violations"]
    assert not wrong and worst < td.SEPARATION
    assert set(res["errors"]) == {"trendCoef[0]", "trendCoef[1]", "varLogDispEsts", "dispPriorVar", "dispFit"}
    assert all(e < td.SEPARATION for e in res["errors"].values()), res["errors"]
    assert (c["S"] - c["p"] <= 3) == (name == "trend-edges-257")  # the simulated prior on one case


def test_tiled_column_has_the_base_statistics(oracle):
    """439 copies of the 599 rows: numpy's median and MAD of the tiled residuals are the base's by bits, and the oracle's coefficients,
    median and MAD on the 262 961 rows pass judge_global against the twin of the 599."""
    b, t = th.edge_case("trend-edges-599"), th.edge_case("trend-edges-tiled")
    _, _, resid = yardstick(oracle, b["baseMean"], b["dispGeneEst"], b["allZero"], b["S"], b["p"])
    x = resid[~np.isnan(resid)]
    xt = np.tile(x, th.TILE_K)
    assert len(x) == 599 - len(b["planted"]["zero"]) - len(b["planted"]["below"]) == 523
    med, medt = np.median(x), np.median(xt)
    mad, madt = np.median(np.abs(x - med)), np.median(np.abs(xt - medt))
    assert td.same_bits(np.array([med, mad]), np.array([medt, madt])).all(), (med, medt, mad, madt)
    fitted, sc, _ = yardstick(oracle, t["baseMean"], t["dispGeneEst"], t["allZero"], t["S"], t["p"])
    res = judge_stage(t, sc, fitted[:599], range(599))
    print(f"tiled: {res['errors']}")
    assert not res["violations"] and res["near"] == 0, res["violations"]
    # The twin's units are those of 599 rows; the glm's sums now run over 439 times as many terms, and a sum of n terms of one sign in any
    # order is within (n - 1) 2^-53 of exact, relative: (n - 1) / 2 units of 2^-52 (measured: 171 and 25 units on the coefficients).  dispFit
    # is a row formula on the reported coefficients and keeps the separation.
    cap = (len(t["baseMean"]) - 1) / 2
    assert res["errors"]["dispFit"] < td.SEPARATION and all(e < cap for e in res["errors"].values()), res["errors"]
