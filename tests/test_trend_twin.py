"""The judge of the trend's other branches and of the simulated prior, and its own test on the CPU.

tests/trend_twin.py restates fitType "mean", fitType "local", the residual rules, the residual histogram and estimateDispersionsPriorVar
for m - p <= 3 in 50-digit arithmetic from the rule texts; judge() holds one set of outputs of the fit's global stage to it on the
columns of a case of tests/trend_inputs.py.  tests/test_gpu_trend.py applies it to the device (chicdiff_hip_selftest_global_stage_dev,
chicdiff_hip_selftest_resid_hist_dev); here it runs on the CPU oracle's routines for the same columns (oracle.local_dispersion_fit,
oracle.mean_dispersion, the oracle's median, oracle.prior_mc_hist / oracle_prior_mc_bin, oracle.prior_var_mc) and on the library's
host forms (chicdiff_hip_selftest_prior_mc) — which must need NO excused decision on the committed inputs —, every wrong reading of a
rule is shown to be rejected, and the table of simulated densities is held to the exact bin probabilities.

Exact on every element: the histogram of the reported residual column, which rows have a NaN residual / a NaN dispFit, the status
bits, trendCoef (NaN, NaN) under a local trend and (mean, 0) under the mean trend, the number of vertices and their order, the argmin
of the prior.  An element may differ from the twin only where the twin holds the deciding comparison inside NEAR_UNITS units of the
values compared and the output agrees with the replay that takes it the other way (a split score against 0.8, a residual against a
fuzzed break in the end-to-end histogram, the argmin's gap); at most EXCUSE_CAP of a case's decisions of that kind.  (A row against a
cell edge is counted as a decision but needs no replay: value and slope are continuous across a vertex, and both sides' formulas agree
there to second order in the distance — far below a unit at NEAR_UNITS units from the edge.)  Everything else: per stratum (quantity,
class) in the units of tests/trend_twin.py.
"""
import math
import time

import mpmath as mp
import numpy as np
import pytest

import disp_twin as dt
import trend_inputs as ti
import trend_twin as tt

SEPARATION = 64.0   # units: between "another formula" and "double arithmetic" (tests/test_disp_twin.py)
EXCUSE_CAP = 0.01   # share of a case's decisions of one kind that may be excused
ST_FAILED, ST_MC, ST_LOCAL = 1, 2, 16
_BITS = ST_FAILED | ST_MC | ST_LOCAL

_EXPECTED = {}


def _f(v):
    return mp.mpf(float(v))


def same_bits(a, b):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return (a.view(np.int64) == b.view(np.int64)) | (np.isnan(a) & np.isnan(b))


# ---------------------------------------------------------------------------------------------------------------------------
# the twin's statement of a case
# ---------------------------------------------------------------------------------------------------------------------------
def expected(case, **wrong):
    """What the rules give on the columns of `case`: dict(error, status, only_status, trend ("local" | "mean" | "supplied"), coefs,
    local (tt.local_trend's result), dispFit / unit_fit per row, resid / unit_resid per row, var = (v, unit), mc, hist = (counts, info),
    prior = tt.prior_var_mc's result | dict(value, unit)).  `wrong`: the keywords of a wrong reading (test_wrong_readings)."""
    key = (case["name"], tuple(sorted((k, str(v)) for k, v in wrong.items())))
    if key in _EXPECTED:
        return _EXPECTED[key]
    w = dict(wrong)
    bm, al, az, S, p, o = case["baseMean"], case["dispGeneEst"], case["allZero"], case["S"], case["p"], case["opts"]
    n = len(bm)
    live = tt.live_rows(bm, al, az)
    E = dict(error=False, status=0, only_status=False, trend=None, coefs=None, local=None, n=n)
    prior_given = "dispPriorVar" in o
    mc = tt.by_simulation(S, p, prior_given, limit=w.pop("sim_limit", 3))
    if mc:
        E["status"] |= ST_MC
    E["mc"] = mc
    fit_type = o.get("fitType", 0)
    with mp.workdps(tt.DPS):
        failed = False
        if "trendCoef" in o:
            c = [_f(v) for v in o["trendCoef"]]
            E.update(trend="supplied", coefs=c)
        elif fit_type == 1:
            mt = tt.mean_trend(al, az, **{k[5:]: w.pop(k) for k in list(w) if k.startswith("mean_")})
            E["mean"] = mt
            if mt["failed"]:
                E["error"] = True
                _EXPECTED[key] = E
                return E
            c = [mt["value"], mp.mpf(0)]
            E.update(trend="mean", coefs=c)
        else:
            if fit_type == 0:
                # the parametric trend of tests/disp_twin.py; without a row to fit there is no trend (a project rule: the status bit)
                try:
                    failed = not live or dt.global_stage([bm[i] for i in live], [al[i] for i in live], 8, 2)["failed"]
                except ArithmeticError:  # a fitted mean <= 0 inside glm: R stops there, and DESeq2 takes that for a failed fit too
                    failed = True
                E["parametric_failed"] = failed
                assert failed, "the stage cases hold no parametric trend that succeeds (tests/test_gpu_disp.py has those)"
            if fit_type == 2 or case["substitute"]:
                lt = tt.local_trend(bm, al, az, **{k[6:]: w.pop(k) for k in list(w) if k.startswith("local_")})
                E["local"] = lt
                failed = lt["failed"] is not None
                if not failed:
                    E["status"] |= ST_LOCAL
                    E.update(trend="local", coefs=None)
        if failed:
            E["status"] |= ST_FAILED
            E["only_status"] = True
            _EXPECTED[key] = E
            return E
        if E["trend"] == "local":
            fit, ufit = E["local"]["dispFit"], E["local"]["unit"]
        else:
            fit, ufit = [None] * n, [None] * n
            for i in live:
                t1 = c[1] / _f(bm[i])
                fit[i] = c[0] + t1
                ufit[i] = (tt.U * (abs(c[0]) + abs(t1))) if E["trend"] == "supplied" else E["mean"]["unit"]
        E.update(dispFit=fit, unit_fit=ufit)
        r, ur = tt.residuals(al, fit, ufit, az, strict=w.pop("resid_strict", False))
        E.update(resid=r, unit_resid=ur)
        have = [i for i in range(n) if r[i] is not None]
        E["var"] = dt.mad_stage({i: r[i] for i in have}, {i: ur[i] for i in have})[::3] if have else None
        hist_kw = {k[5:]: w.pop(k) for k in list(w) if k.startswith("hist_")}
        E["hist"] = tt.resid_hist(r, ur, **hist_kw) if mc else ([0] * 40, [])
        if prior_given:
            E["prior"] = dict(value=_f(o["dispPriorVar"]), unit=mp.mpf(0), closed_form=True)
        elif mc and 1 <= S - p <= 3:
            kw = {k[6:]: w.pop(k) for k in list(w) if k.startswith("prior_")}
            if kw.pop("all_residuals", False):
                kw["all_count"] = len(have)
            E["prior"] = tt.prior_var_mc(E["hist"][0], tt.simulated_densities(S - p), S - p, var_log_disp_ests=E["var"][0] if have else None, **kw)
            if E["prior"]["closed_form"]:
                E["prior"]["unit"] = E["var"][1] + tt.U * (E["var"][0] + mp.polygamma(1, mp.mpf(S - p) / 2))
        elif mc:
            E["prior"] = None  # (a wrong reading that simulates where no table exists: the status bit and the counts show it)
        else:
            v, uv = E["var"]
            tri = mp.polygamma(1, mp.mpf(S - p) / 2)
            pv = v - tri
            E["prior"] = dict(value=pv if pv > mp.mpf(0.25) else mp.mpf(0.25), unit=uv + tt.U * (v + tri), closed_form=True)
    assert not w, ("unknown wrong-reading keywords", w)
    _EXPECTED[key] = E
    return E


def as_outputs(case, E):
    """The twin's statement rounded to doubles, in the shape of a set of outputs (what a correct — or, from a wrong reading, an
    incorrect — implementation would report)."""
    n = len(case["baseMean"])
    nan = float("nan")
    out = dict(error=E["error"], status=E["status"], trendCoef=(nan, nan), dispFit=np.full(n, nan), resid=np.full(n, nan), hist=np.zeros(40),
               vertices=dict(nv=0, x=np.zeros(0), h=np.zeros(0), f=np.zeros(0), d=np.zeros(0)), varLogDispEsts=nan, dispPriorVar=nan)
    if E["error"] or E["only_status"]:
        return out
    if E["coefs"] is not None:
        out["trendCoef"] = (float(E["coefs"][0]), float(E["coefs"][1]))
    if E["trend"] == "local":
        vs = E["local"]["vertices"]
        out["vertices"] = dict(nv=len(vs), **{k: np.array([float(v[k]) for v in vs]) for k in "xhfd"})
        out["dispFit"] = np.array([nan if v is None else float(v) for v in E["dispFit"]])
    out["resid"] = np.array([nan if v is None else float(v) for v in E["resid"]])
    out["hist"] = np.array(E["hist"][0], dtype=np.float64)
    if E["var"] is not None:
        out["varLogDispEsts"] = float(E["var"][0])
    if E["prior"] is not None:
        out["dispPriorVar"] = float(E["prior"]["value"])
    out["hist_of_resid"] = np.array(tt.resid_hist(out["resid"])[0], dtype=np.float64)
    return out


# ---------------------------------------------------------------------------------------------------------------------------
# the judge
# ---------------------------------------------------------------------------------------------------------------------------
def _err(res, quantity, cls, got, exact, unit, row=-1):
    e = float(abs(_f(got) - exact) / unit) if unit > 0 else (0.0 if _f(got) == exact else math.inf)
    res["errors"].setdefault((quantity, cls), []).append((e, row))


def judge(case, out):
    res = _judge(case, out)
    for k, v in res["excused"].items():
        if v > EXCUSE_CAP * res["decisions"].get(k, 0):
            res["violations"].append((f"excused decisions of kind '{k}' beyond the cap", (v, res["decisions"].get(k, 0))))
    return res


def _judge(case, out):
    """Holds `out` — dict(error, status, trendCoef, dispFit[n], resid[n], hist[40], hist_of_resid[40] (the histogram routine on the
    reported residual column), vertices = dict(nv, x, h, f, d), varLogDispEsts, dispPriorVar) — to the twin on the case's columns.
    Returns dict(violations = [(what, detail)], errors = {(quantity, class): [(error in units, row)]}, decisions = {kind: count},
    near = {kind: decisions inside NEAR_UNITS units}, excused = {kind: count})."""
    E = expected(case)
    res = dict(violations=[], errors={}, decisions={}, near={}, excused={})
    bad = res["violations"].append
    if bool(out["error"]) != E["error"]:
        bad(("error", (bool(out["error"]), E["error"])))
    if E["error"] or out["error"]:
        return res
    if int(out["status"]) & _BITS != E["status"]:
        bad(("status bits", (int(out["status"]) & _BITS, E["status"])))
    if E["only_status"]:
        return res
    bm, al, n = case["baseMean"], case["dispGeneEst"], E["n"]
    with mp.workdps(tt.DPS):
        tc = [float(v) for v in out["trendCoef"]]
        # ---- the trend ----
        if E["trend"] == "local":
            if not (tc[0] != tc[0] and tc[1] != tc[1]):
                bad(("trendCoef under a local trend", tc))
            L = _judge_vertices(case, E, out, res) if "vertices" in out else E["local"]  # (a fit does not report its vertices)
            if L is None:
                return res
            got = np.asarray(out["dispFit"], dtype=np.float64)
            want_nan = np.array([v is None for v in L["dispFit"]])
            if not np.array_equal(np.isnan(got), want_nan):
                bad(("rows with a NaN dispFit", np.flatnonzero(np.isnan(got) != want_nan)[:10].tolist()))
                return res
            edges = [i for i in range(n) if L["edge"][i] is not None]
            res["decisions"]["cell edge"] = len(edges)
            res["near"]["cell edge"] = sum(1 for i in edges if L["edge"][i][0] <= tt.NEAR_UNITS * L["edge"][i][1])
            for i in range(n):
                if L["dispFit"][i] is not None:
                    _err(res, "dispFit", L["cls"][i], got[i], L["dispFit"][i], L["unit"][i], i)
            fit_ref = {i: (_f(got[i]), mp.mpf(0)) for i in range(n) if not want_nan[i]}
        else:
            if E["trend"] == "mean":
                if tc[1] != 0.0:
                    bad(("trendCoef[1] under the mean trend", tc[1]))
                _err(res, "mean trend", "all", tc[0], E["coefs"][0], E["mean"]["unit"])
            elif not (same_bits(tc[0], float(E["coefs"][0])) and same_bits(tc[1], float(E["coefs"][1]))):
                bad(("supplied trendCoef", tc))
            c0, c1 = _f(tc[0]), _f(tc[1])
            fit_ref = {}
            for i in tt.live_rows(bm, al, case["allZero"]):
                t1 = c1 / _f(bm[i])
                fit_ref[i] = (c0 + t1, tt.U * (abs(c0) + abs(t1)) if c1 != 0 else mp.mpf(0))
        # ---- residuals: the pattern against the twin, the values against the REPORTED trend (the row formula on its own inputs) ----
        if "resid" not in out:  # (a fit reports no residuals: the scalars alone)
            return _judge_scalars(E, out, res)
        r = np.asarray(out["resid"], dtype=np.float64)
        want_nan = np.array([v is None for v in E["resid"]])
        if not np.array_equal(np.isnan(r), want_nan):
            bad(("rows with a NaN residual", np.flatnonzero(np.isnan(r) != want_nan)[:10].tolist()))
            return res
        for i in np.flatnonzero(~want_nan):
            f_, uf = fit_ref[int(i)]
            lg, lf = mp.log(_f(al[i])), mp.log(f_)
            _err(res, "residual", E["trend"], r[i], lg - lf, tt.U * (abs(lg) + abs(lf)) + uf / f_, int(i))
        # ---- the histogram routine on the reported column: comparisons of doubles, no allowance ----
        direct = tt.resid_hist(r)[0]
        if "hist_of_resid" in out and not np.array_equal(np.asarray(out["hist_of_resid"]), np.array(direct, dtype=np.float64)):
            bad(("histogram of the reported residuals", (np.asarray(out["hist_of_resid"]) - np.array(direct)).tolist()))
        # ---- the end-to-end histogram: the twin's residuals, a residual near a fuzzed break may fall either way ----
        counts, info = E["hist"]
        res["decisions"]["break"] = len(info)
        nearb = [(i, j, d, u) for i, j, d, u in info if d <= tt.NEAR_UNITS * u]
        res["near"]["break"] = len(nearb)
        diff = np.asarray(out["hist"], dtype=np.float64) - np.array(counts, dtype=np.float64)
        if diff.any():
            fb = [_f(v) for v in tt.fuzzed_breaks()]
            moved = 0
            for i, j, d, u in nearb:
                if j < 0:
                    continue
                xv = E["resid"][i]
                to = j - 1 if (j > 0 and abs(xv - fb[j]) == d) else j + 1 if (j < 39 and abs(xv - fb[j + 1]) == d) else None
                if to is not None and diff[j] < 0 and diff[to] > 0:
                    diff[j] += 1
                    diff[to] -= 1
                    moved += 1
            res["excused"]["break"] = moved
            if diff.any():
                bad(("end-to-end histogram", diff.tolist()))
        _judge_scalars(E, out, res)
    return res


def _judge_scalars(E, out, res):
    """varLogDispEsts and dispPriorVar (inside the caller's workdps)."""
    bad = res["violations"].append
    if E["var"] is not None:
        _err(res, "varLogDispEsts", E["trend"], out["varLogDispEsts"], E["var"][0], E["var"][1])
    P = E["prior"]
    if P is not None:
        pv = float(out["dispPriorVar"])
        if P.get("closed_form"):
            _err(res, "dispPriorVar", "closed form", pv, P["value"], P["unit"])
        else:
            res["decisions"]["argmin"] = 1
            gap, ug = P["gap"]
            res["near"]["argmin"] = int(gap <= tt.NEAR_UNITS * ug)
            if not same_bits(pv, float(P["value"])):
                other = max(tt.grid_x(P["runner_up"], tt.FINE), mp.mpf(0.25))
                if res["near"]["argmin"] and same_bits(pv, float(other)):
                    res["excused"]["argmin"] = 1
                else:
                    bad(("argmin of the prior", (pv, float(P["value"]), P["argmin"], P["runner_up"], float(gap / ug))))
    return res


def _judge_vertices(case, E, out, res):
    """The number of vertices, their order and their values; returns the replay the outputs follow (the twin's own, or the one with a
    near split taken the other way), None when they follow neither."""
    L = E["local"]
    V = out["vertices"]
    splits = L["decisions"]
    res["decisions"]["split"] = len(splits)
    near = [k for k, d in enumerate(splits) if abs(d["margin"]) <= tt.NEAR_UNITS * d["unit"]]
    res["near"]["split"] = len(near)
    x = np.asarray(V["x"], dtype=np.float64)
    if int(V["nv"]) != len(x) or (len(x) > 1 and not (np.diff(x) > 0).all()):
        res["violations"].append(("vertices not in ascending order", x.tolist()))
        return None

    def follows(lt):
        return lt["failed"] is None and len(lt["vertices"]) == len(x) and all(abs(_f(a) - v["x"]) <= SEPARATION * v["u_x"] for a, v in zip(x, lt["vertices"]))
    if not follows(L):
        for k in near:
            alt = tt.local_trend(case["baseMean"], case["dispGeneEst"], case["allZero"], flip=(k,))
            if follows(alt):
                res["excused"]["split"] = 1
                L = alt
                break
        else:
            res["violations"].append(("number / positions of the vertices", (len(x), len(L["vertices"]))))
            return None
    for j, v in enumerate(L["vertices"]):
        for q in "xhfd":
            _err(res, f"vertex {q}", "end" if j in (0, len(x) - 1) else "inner", V[q][j], v[q], v["u_" + q], j)
    return L


def worst(res):
    return {k: max(v) for k, v in res["errors"].items()}


def rejected(res, bound=SEPARATION):
    return bool(res["violations"]) or any(e > bound for v in res["errors"].values() for e, _ in v)


# ---------------------------------------------------------------------------------------------------------------------------
# the oracle's routines and the library's host forms on the columns of a case
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def oracle():
    from oracle import oracle as o
    o.build()
    return o


def host_prior_var(hist, df):
    """chicdiff_hip_selftest_prior_mc: the library's host form of the simulated prior (pmc_prior_var)."""
    import ctypes as C
    from chicdiff_amd import hip
    h = np.ascontiguousarray(hist, dtype=np.float64)
    pv = C.c_double(0.0)
    assert hip.load_library().chicdiff_hip_selftest_prior_mc(int(df), h.ctypes.data_as(C.c_void_p), None, C.byref(pv)) == 0
    return pv.value


def oracle_outputs(oracle, case, host_forms=False):
    """The stage as the oracle's routines give it on the case's columns (the yardstick of tests/test_gpu_trend.py).  host_forms: the
    prior from the library's host entry instead of the oracle's."""
    bm, al, az, S, p, o = case["baseMean"], case["dispGeneEst"], case["allZero"], case["S"], case["p"], case["opts"]
    n = len(bm)
    nan = float("nan")
    live = az == 0
    out = dict(error=False, status=0, trendCoef=(nan, nan), dispFit=np.full(n, nan), resid=np.full(n, nan), hist=np.zeros(40),
               vertices=dict(nv=0, x=np.zeros(0), h=np.zeros(0), f=np.zeros(0), d=np.zeros(0)), varLogDispEsts=nan, dispPriorVar=nan)
    mc = "dispPriorVar" not in o and 0 < S - p <= 3
    if mc:
        out["status"] |= ST_MC
    fit_type = o.get("fitType", 0)
    with np.errstate(invalid="ignore", divide="ignore"):
        use = live & (al > 100 * ti.MIN_DISP)
        failed = local = False
        if "trendCoef" in o:
            c = tuple(float(v) for v in o["trendCoef"])
        elif fit_type == 1:
            m = oracle.mean_dispersion(al[live])
            if m is None:
                out["error"] = True
                return out
            c = (m, 0.0)
        else:
            if fit_type == 0:
                failed = not use.any() or oracle.parametric_dispersion_fit(bm[use], al[use])[2] != 0
                assert failed
            if fit_type == 2 or case["substitute"]:
                try:
                    vert, pred = oracle.local_dispersion_fit(bm[use], al[use])
                    failed, local = False, True
                except RuntimeError:
                    failed = True
        if failed:
            out["status"] |= ST_FAILED
            return out
        if local:
            out["status"] |= ST_LOCAL
            out["vertices"] = dict(nv=len(vert["x"]), **vert)
            out["dispFit"][live] = np.exp(pred(np.log(bm[live])))
            fitted = out["dispFit"]
        else:
            out["trendCoef"] = c
            fitted = c[0] + c[1] / bm
        keep = live & (al >= 100 * ti.MIN_DISP)
        out["resid"][keep] = np.log(al[keep]) - np.log(fitted[keep])
    x = np.ascontiguousarray(out["resid"][keep])
    lib = oracle.lib()
    out["hist_of_resid"] = np.bincount([b for b in (lib.oracle_prior_mc_bin(float(v)) for v in x) if b >= 0], minlength=40).astype(np.float64)
    assert np.array_equal(out["hist_of_resid"], oracle.prior_mc_hist(x))
    if mc:
        out["hist"] = out["hist_of_resid"].copy()
    if len(x):
        med = lib.oracle_median(oracle._pd(x.copy()), len(x))
        dev = np.ascontiguousarray(np.abs(x - med))
        out["varLogDispEsts"] = (1.4826 * lib.oracle_median(oracle._pd(dev), len(x))) ** 2
    closed = max(out["varLogDispEsts"] - lib.oracle_trigamma((S - p) / 2.0), 0.25)
    if "dispPriorVar" in o:
        out["dispPriorVar"] = float(o["dispPriorVar"])
    elif mc and out["hist"].sum() > 0:
        out["dispPriorVar"] = host_prior_var(out["hist"], S - p) if host_forms else lib.oracle_prior_var_mc(oracle._pd(out["hist"]), S - p)
    else:
        out["dispPriorVar"] = closed
    return out


_CASES = {c["name"]: c for c in ti.stage_cases()}


def report(name, res):
    for k, (e, row) in sorted(worst(res).items()):
        print(f"  {name} | {k[0]} | {k[1]}: n={len(res['errors'][k])} worst {e:.3g} units (row {row})")
    print(f"  {name} | decisions {res['decisions']} near {res['near']} excused {res['excused']}")


@pytest.mark.parametrize("name", list(_CASES))
def test_oracle_and_host_forms_against_twin(oracle, name):
    """The oracle's routines and the library's host forms on every stage case: no violation, NO excused decision (the condition the
    inputs are chosen to meet), every stratum below SEPARATION units; the twin's own statement, rounded to doubles, passes too."""
    case = _CASES[name]
    t0 = time.perf_counter()
    E = expected(case)
    for label, out in (("oracle", oracle_outputs(oracle, case)), ("host forms", oracle_outputs(oracle, case, host_forms=True)),
                       ("twin, rounded", as_outputs(case, E))):
        res = judge(case, out)
        report(f"{name} [{label}]", res)
        assert not res["violations"], (label, res["violations"][:5])
        assert not any(res["excused"].values()), (label, res["excused"])
        assert all(e < SEPARATION for e, _ in worst(res).values()), (label, {k: v for k, v in worst(res).items() if not v[0] < SEPARATION})
    print(f"  {name}: {time.perf_counter() - t0:.1f} s; status {E['status']}" + (f", local trend: {E['local']['failed'] or len(E['local']['vertices'])}" if E.get("local") else ""))


def test_planted_edges_are_present():
    """What the cases are built to hold, as the twin sees it."""
    with mp.workdps(tt.DPS):
        E = expected(_CASES["local-wide-S8p2"])
        L = E["local"]
        cls = [c for c in L["cls"] if c]
        assert cls.count("left") >= 3 and cls.count("right") >= 3 and cls.count("vertex") >= 7 and cls.count("interior") >= 400, {c: cls.count(c) for c in set(cls)}
        assert len(L["vertices"]) >= 4 and L["k"] == 350 and L["nfit"] == 501
        case = _CASES["local-wide-S8p2"]
        al = case["dispGeneEst"]
        for thr, rule in ((ti.T100, None), (ti.T10, None)):
            for v in (np.nextafter(thr, 0.0), thr, np.nextafter(thr, 1.0)):
                assert (al == v).sum() == 1
        # the boundary row is in the residuals and not in the fit
        i = int(np.flatnonzero(al == ti.T100)[0])
        assert E["resid"][i] is not None and E["resid"][int(np.flatnonzero(al == np.nextafter(ti.T100, 0.0))[0])] is None
        assert tt.local_trend(case["baseMean"], al, case["allZero"], strict=False)["nfit"] == 502
        # ties at rank k: from the end vertices, rows sit at |dx| = h exactly
        x = sorted(mp.log(_f(case["baseMean"][j])) for j in tt.live_rows(case["baseMean"], al, case["allZero"]) if al[j] > ti.T100)
        for v in (L["vertices"][0], L["vertices"][-1]):
            assert sum(1 for a in x if abs(a - v["x"]) == v["h"]) >= 3
        assert [expected(_CASES[f"mean-{u}"])["mean"]["lo"] for u in (999, 1000, 1001, 1999, 2000)] == [0, 1, 1, 1, 2]
        assert [expected(_CASES[f"mean-{u}"])["mean"]["n"] for u in (999, 1000, 1001, 1999, 2000)] == [999, 1000, 1001, 1999, 2000]
        assert expected(_CASES["mean-none-usable"])["error"]
        reasons = {k: expected(_CASES[k])["local"]["failed"] for k in ("local-nfit3", "local-nfit4", "local-n1", "local-equal-means", "local-h0")}
        assert reasons == {"local-nfit3": "fewer than four rows", "local-nfit4": "singular system", "local-n1": "fewer than four rows",
                           "local-equal-means": "max x = min x", "local-h0": "h = 0"}, reasons
        assert expected(_CASES["param-fails-coef-substituted"])["status"] == ST_LOCAL and expected(_CASES["param-fails-coef-reported"])["status"] == ST_FAILED
        assert expected(_CASES["param-fails-rounds-substituted"])["status"] == ST_LOCAL
        for name, by_coef in (("param-fails-coef-substituted", True), ("param-fails-rounds-substituted", False)):  # the two ways to fail
            c = _CASES[name]
            rows = tt.live_rows(c["baseMean"], c["dispGeneEst"], c["allZero"])
            gs = dt.global_stage([c["baseMean"][i] for i in rows], [c["dispGeneEst"][i] for i in rows], 8, 2)
            assert gs["failed"] and (not (gs["coefs"][0] > 0 and gs["coefs"][1] > 0)) == by_coef, (name, gs["coefs"])
            assert gs["near"] > 1e-9, (name, gs["near"])  # no filter bound or stop test decides within rounding
        # the simulated prior: an argmin at 0, below and above the floor, interior, at the grid's end
        arg = {v: expected(_CASES[f"prior-S4-2v2-v{v:g}"])["prior"]["argmin"] for v in ti.PRIOR_V}
        print("  argmin by v (d.f. 2):", arg)
        assert arg[0.0] == 0 and any(0 < a < 32 for a in arg.values()) and arg[12.0] == tt.FINE - 1 and any(32 <= a < tt.FINE - 1 for a in arg.values())
        assert expected(_CASES["prior-none-inside"])["prior"]["closed_form"] and sum(expected(_CASES["prior-none-inside"])["hist"][0]) == 0
        assert sum(1 for c in expected(_CASES["prior-one-bin"])["hist"][0] if c) == 1
        h = expected(_CASES["prior-extreme-bins"])["hist"][0]
        assert h[0] > 0 and h[39] > 0 and sum(h[1:39]) == 0
        assert expected(_CASES["prior-df4-S6p2"])["status"] == 0


# ---------------------------------------------------------------------------------------------------------------------------
# the judge can fail: the wrong readings
# ---------------------------------------------------------------------------------------------------------------------------
WRONG = {
    ">= for > in the fit's row rule": ("local-wide-S8p2", dict(local_strict=False)),
    "> for >= in the residuals' row rule": ("local-wide-S8p2", dict(resid_strict=True)),
    "100 minDisp for 10 minDisp in the mean": ("mean-1000", dict(mean_factor=100)),
    "an untrimmed mean": ("mean-1000", dict(mean_trim=0.0)),
    "ceil for floor in the trim count": ("mean-1001", dict(mean_count=math.ceil)),
    "round for floor in the trim count": ("mean-1999", dict(mean_count=round)),
    "ceil for floor in k": ("local-n255", dict(local_kfun=math.ceil)),
    "round for floor in k": ("local-n256", dict(local_kfun=round)),
    "a fit without the baseMean weights": ("local-wide-S8p2", dict(local_weights=False)),
    "bisquare for tricube": ("local-wide-S8p2", dict(local_kernel="bisquare")),
    "cut = 1.0": ("local-dense-centre", dict(local_cut=1.0)),
    "a constant continuation outside the range": ("local-wide-S8p2", dict(local_linear_outside=False)),
    "Hermite slopes not scaled by the cell width": ("local-wide-S8p2", dict(local_scale_slopes=False)),
    # (a residual of a fit is a difference of two logarithms of doubles: it never IS a break, so left-closed bins cannot show through
    # columns; a missing fuzz can — a residual inside (brk, brk + 5e-8] — but no committed case holds one: both are shown on the routine)
    "left-closed bins": (None, dict(right=False)),
    "no fuzz": (None, dict(fuzz=0.0)),
    "densities normalised by all residuals": ("prior-many-outside", dict(prior_all_residuals=True)),
    "small from the observed side only": ("prior-S4-2v2-v1", dict(prior_small_from="observed")),
    "KL with the two densities exchanged": ("prior-S4-2v2-v1", dict(prior_exchanged=True)),
    "loess span 0.75": ("prior-S4-2v2-v1", dict(prior_span=0.75)),
    "loess degree 1": ("prior-S4-2v2-v1", dict(prior_degree=1)),
    # ("the last minimum for the first" cannot show on columns: test_last_minimum_needs_a_plateau)
    "no 0.25 floor": ("prior-S4-2v2-v0.1", dict(prior_floor=False)),
    "simulation at m - p < 3 only": ("prior-S4~1-v1", dict(sim_limit=2)),
    "simulation at m - p = 4": ("prior-df4-S6p2", dict(sim_limit=4)),
}


@pytest.mark.parametrize("reading", list(WRONG))
def test_wrong_readings_are_rejected(reading):
    """Each wrong reading of a rule, stated by the twin itself and rounded to doubles, is rejected by the judge on the case named,
    where the right reading passes (test_oracle_and_host_forms_against_twin)."""
    name, kw = WRONG[reading]
    if name is None:  # a reading of the histogram rule: the routine on a residual column that holds the breaks themselves
        x = ti.hist_edge_values()
        assert judge_hist(x, tt.resid_hist(x, **kw)[0]), reading
        assert not judge_hist(x, tt.resid_hist(x)[0])
        return
    case = _CASES[name]
    res = judge(case, as_outputs(case, expected(case, **kw)))
    print(f"  {reading} on {name}: violations {res['violations'][:2]}, worst {sorted(worst(res).items(), key=lambda t: -t[1][0])[:2]}")
    assert rejected(res), reading
    right = judge(case, as_outputs(case, expected(case)))
    assert not rejected(right) and not any(right["excused"].values())


def judge_hist(x, counts):
    """The histogram routine on a residual column: the twin's counts on the same doubles, exactly.  Returns the violations."""
    want = tt.resid_hist(x)[0]
    return [] if list(np.asarray(counts, dtype=np.float64)) == [float(c) for c in want] else [("histogram of a residual column", (np.asarray(counts) - np.array(want)).tolist())]


def test_last_minimum_needs_a_plateau():
    """'The last minimum for the first' shows only where two fitted values are equal: a single residual gives KL sums whose loess has no
    such tie in 50 digits, so on the committed inputs this reading cannot show through the data.  It shows on the rule itself: a
    fitted curve with a plateau."""
    with mp.workdps(tt.DPS):
        fitted = [mp.mpf(1)] * tt.FINE
        fitted[100] = fitted[200] = mp.mpf(0)
        first = [f for f in range(tt.FINE) if fitted[f] == min(fitted)]
        assert first[0] == 100 and first[-1] == 200


# ---------------------------------------------------------------------------------------------------------------------------
# KL sums and loess values of the oracle; the histogram routine on the edge values
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["prior-S3p2-v0.3", "prior-S4-2v2-v1", "prior-S4~1-v8", "prior-one-residual", "prior-extreme-bins"])
def test_kl_and_loess_of_the_oracle(oracle, name):
    """The 200 KL sums and the 1 000 loess values of oracle.prior_var_mc against the twin's, in their units (the loess values from
    the oracle's own KL sums, so that the stratum holds the operator alone)."""
    case = _CASES[name]
    E = expected(case)
    with mp.workdps(tt.DPS):
        pv, kl, fit = oracle.prior_var_mc_trace(np.array(E["hist"][0], dtype=np.float64), case["S"] - case["p"])
        P = E["prior"]
        e_kl = max(float(abs(_f(kl[g]) - P["kl"][g]) / P["kl_unit"][g]) for g in range(tt.GRID))
        ref, unit = tt.loess_fitted(kl)
        e_lo = max(float(abs(_f(fit[f]) - ref[f]) / unit[f]) for f in range(tt.FINE))
    print(f"  {name}: KL worst {e_kl:.3g} units, loess worst {e_lo:.3g} units, argmin {P['argmin']}, gap {float(P['gap'][0] / P['gap'][1]):.3g} units")
    assert e_kl < SEPARATION and e_lo < SEPARATION
    assert same_bits(pv, float(P["value"]))


def test_histogram_rule_on_the_edge_values(oracle):
    """oracle_prior_mc_bin (the oracle's statement of pmc_bin) and oracle.prior_mc_hist on every fuzzed break, its neighbours, the
    breaks themselves, +-10, +-Inf, NaN and +-0: the twin's counts, exactly."""
    x = ti.hist_edge_values()
    want, info = tt.resid_hist(x, [0] * len(x))  # (units given: the element-wise statement, with each element's bin)
    assert want == tt.resid_hist(x)[0]
    lib = oracle.lib()
    got = np.bincount([b for b in (lib.oracle_prior_mc_bin(float(v)) for v in x) if b >= 0], minlength=40)
    assert got.tolist() == want
    finite = x[np.isfinite(x)]
    assert oracle.prior_mc_hist(finite).tolist() == tt.resid_hist(finite)[0]
    bins = {i: j for i, j, _, _ in info}
    for j in range(1, 40):  # the fuzzed break itself belongs to the bin below, its upper neighbour to the bin above
        fb = (j / 2.0 - 10.0) + 5e-8
        i = int(np.flatnonzero(x == fb)[0])
        assert bins[i] == j - 1 and bins[int(np.flatnonzero(x == np.nextafter(fb, np.inf))[0])] == j
    for n in ti.HIST_SIZES:
        col = ti.hist_column(n)
        assert len(col) == n


# ---------------------------------------------------------------------------------------------------------------------------
# one more pin of the table: the simulated densities against the exact bin probabilities
# ---------------------------------------------------------------------------------------------------------------------------
def exact_bin_probabilities(df, v, nodes=200):
    """P(fb_j < log(chi2_df / df) + N(0, v) <= fb_j+1) for the 40 bins and the mass outside (-10, 10): the chi-square distribution
    function under a Gauss-Hermite rule over the normal part."""
    from scipy.stats import chi2
    fb = np.array(tt.fuzzed_breaks())
    fb[0], fb[-1] = -10.0, 10.0
    if v == 0:
        cdf = chi2.cdf(df * np.exp(fb), df)
    else:
        t, w = np.polynomial.hermite_e.hermegauss(nodes)
        w = w / w.sum()
        cdf = (chi2.cdf(df * np.exp(fb[:, None] - math.sqrt(v) * t[None, :]), df) * w[None, :]).sum(axis=1)
    p = np.diff(cdf)
    return p / p.sum()


@pytest.mark.parametrize("df", [1, 2, 3])
def test_simulated_densities_fit_the_exact_bin_probabilities(df):
    """The 200 simulated densities of one d.f. (10 000 draws each, R's stream under set.seed(2): deterministic) against the exact bin
    probabilities of log(chi2_df / df) + N(0, v) truncated to (-10, 10): Pearson's statistic per variance, bins pooled from both tails
    inward until the expected count is >= 10; every p-value >= 1e-5 (Bonferroni over the 600: a false alarm in 0.6 %), and the 200
    p-values uniform by Kolmogorov-Smirnov at p >= 0.01.  (The KS test on the chi-square scale in tests/test_r_rng.py cannot see what
    rgamma does below e^-10; this can: at d.f. 1, 1.3 % of the draws fall outside the histogram on that side.)"""
    from scipy import stats
    dens = tt.simulated_densities(df)
    pvals = []
    for g in range(200):
        v = 8.0 * g / 199
        d = dens[g]
        # counts = dens * 0.5 * inside, integers: inside is the largest number of draws <= 10 000 that makes them so
        m1 = 2.0 / d[d > 0].min()  # ... if the smallest positive count is 1; else a divisor of it
        inside = next(m for m in (int(round(m1 * c)) for c in range(int(10000 / m1) + 1, 0, -1))
                      if m <= 10000 and np.abs(d * 0.5 * m - np.round(d * 0.5 * m)).max() < 1e-6)
        cnt = np.round(d * 0.5 * inside)
        assert cnt.sum() == inside and inside > 9000
        exp = exact_bin_probabilities(df, v) * inside
        o_, e_ = list(cnt), list(exp)
        while e_[0] < 10 or e_[1] < 10:  # (inward: until the pooled class and the bin behind it both hold 10)
            o_[:2], e_[:2] = [o_[0] + o_[1]], [e_[0] + e_[1]]
        while e_[-1] < 10 or e_[-2] < 10:
            o_[-2:], e_[-2:] = [o_[-2] + o_[-1]], [e_[-2] + e_[-1]]
        o_, e_ = np.array(o_), np.array(e_)
        keep = e_ >= 10  # (inner bins below 10 do not occur: the densities are unimodal)
        assert keep.all()
        x2 = ((o_ - e_) ** 2 / e_).sum()
        pvals.append(stats.chi2.sf(x2, len(e_) - 1))
    pvals = np.array(pvals)
    ks = stats.kstest(pvals, "uniform").pvalue
    print(f"  d.f. {df}: smallest p {pvals.min():.3g}, KS p {ks:.3g}")
    assert pvals.min() >= 1e-5, (df, int(pvals.argmin()), pvals.min())
    assert ks >= 0.01, (df, ks)
