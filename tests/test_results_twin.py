"""The results stage under an exact judge: Cook's filter, independent filtering (theta, type-7 cuts, the 50 BH rejection counts, lowess,
the threshold rule, the final padj), p.adjust("BH") and the IHW application, on the small cases of tests/results_inputs.py.

Until here this stage was held to tests/results_twin.py — the project's own numpy restatement, same formulas, same precision, same
author — at rtol = 1e-13 on continuous random inputs, and to one real table that always chooses filter 6.  tests/results_exact_twin.py
shares no code with either and works in exact rationals and 50 digits; this module puts

  * tests/results_twin.py and oracle.bh_adjust / oracle.ihw_apply under it (the YARDSTICK of tests/test_gpu_results.py): the exact
    requirements on every element — the NA pattern of padj; which rows Cook's filter sets to NA; numRej[f] equal to the IEEE sequence
    fl(fl(m / r) p) < alpha for every filter whose cut has no baseMean inside its band, and equal to it under one of the two
    readings (band rows all pass / all fail) for the others; the chosen index wherever every decision leading to it has a margin
    above SEPARATION units; padj and weighted_padj bit for bit the IEEE BH sequence over the rows they were given; equal padj on
    tied p-values; the IHW group wherever log|avDist| is more than 2 ulp from a break — and per stratum the value errors of theta,
    filterThreshold, lowess, weight and weighted_pvalue below SEPARATION units (not an accuracy claim);
  * eighteen wrong readings, each a variant of a plain restatement built from the twin's own pieces, under the same judge: each must
    be rejected on a planted case the right reading passes — with one exception, stated where it is tested: `numRej >= thresh` for
    `>` parts from the right reading only where thresh equals an integer exactly, which no double evaluation of lowess decides.

A decision excused (a differing index with a near decision behind it; a group within 2 ulp of a break) is counted and capped at NEAR_CAP
of the case's decisions of that kind.
"""
import math
from fractions import Fraction

import mpmath as mp
import numpy as np
import pytest

import results_exact_twin as rx
import results_inputs as ri
import results_twin as yard
from test_norm_twin import Verdict, same_bits
from test_wald_twin import NEAR_CAP, SEPARATION

GROUP_ULPS = 2.0


@pytest.fixture(scope="module")
def oracle():
    import __graft_entry__ as g
    g.build()
    from oracle import oracle as o
    return o


def mpf_of(fr):
    return mp.mpf(fr.numerator) / fr.denominator


_TWIN = {}


def twin_of(key, make):
    if key not in _TWIN:
        _TWIN[key] = make()
    return _TWIN[key]


def if_twin(case):
    def make():
        c = rx.cuts(case["baseMean"])
        return c, rx.num_rej_readings(case["baseMean"], case["pvalue"], case["alpha"], c)
    return twin_of(("if", case["name"]), make)


# ---------------------------------------------------------------------------------------------------------------------------
# the judge
# ---------------------------------------------------------------------------------------------------------------------------
def judge_bh(v, what, p, padj):
    """padj bit for bit the IEEE sequence over p; equal padj on tied p"""
    want = np.array(rx.bh_ieee([float(x) for x in p]))
    bad = np.flatnonzero(~same_bits(padj, want))
    for i in bad[:5]:
        v.violations.append((what, int(i), float(padj[i]), float(want[i])))
    ok = ~np.isnan(p)
    o = np.argsort(np.asarray(p)[ok], kind="stable")
    ps, qs = np.asarray(p)[ok][o], np.asarray(padj)[ok][o]
    tied = np.flatnonzero((np.diff(ps) == 0) & ~same_bits(qs[1:], qs[:-1]))
    for i in tied[:5]:
        v.violations.append((what + ": tied p, different padj", int(i), float(qs[i]), float(qs[i + 1])))


def judge_filtering(case, padj, info):
    """Returns a Verdict with .stats: decisions taken another way than exact arithmetic takes them, excused ones, the planted edge."""
    v = Verdict()
    name, bm, p, alpha = case["name"], case["baseMean"], case["pvalue"], case["alpha"]
    c, rd = if_twin(case)
    st = v.stats = dict(band_filters=sum(1 for b in c["band"] if b), band_taken_other=[], index_decisions=0, index_near=0, index_excused=0,
                        ieee_exact_disagree=sum(r["disagree"] for r in rd), near_int_h=sum(c["near_int"]))
    with mp.workdps(rx.DPS):
        for k in range(rx.NQ):
            v.value(("theta", "all"), k, info["theta"][k], mpf_of(c["theta"][k]), mpf_of(c["theta_unit"][k]))
        nr = [int(x) for x in info["numRej"]]
        for f in range(rx.NQ):
            if float(info["numRej"][f]) != nr[f] or nr[f] not in rd[f]["ieee"]:
                v.violations.append(("numRej", f, float(info["numRej"][f]), rd[f]["ieee"]))
            elif len(rd[f]["ieee"]) == 2 and rd[f]["ieee"][0] != rd[f]["ieee"][1]:
                exact_reading = 1 if all(b >= c["cut"][f] for b in c["band"][f]) else 0
                if nr[f] != rd[f]["ieee"][exact_reading]:
                    st["band_taken_other"].append((f, float(abs(c["band"][f][0] - c["cut"][f]) / c["unit"][f])))
        ch = twin_of(("choose", name, tuple(nr)), lambda: rx.choose(c["theta"], nr))
        near = [d for d in ch["decisions"] if d[1] <= SEPARATION]
        st["index_decisions"], st["index_near"] = len(ch["decisions"]), len(near)
        j = int(info["index"]) - 1
        if int(info["index"]) != ch["index"]:
            if near and 0 <= j < rx.NQ:
                st["index_excused"] = 1
                st["index_margin"] = min(d[1] for d in near)
            else:
                v.violations.append(("index", 0, int(info["index"]), ch["index"]))
                j = min(max(j, 0), rx.NQ - 1)
        st["lowess_ill"] = ch["ill"]   # see UNITS in results_exact_twin.py: then the fitted values are no requirement
        cls = "all four passes" if ch["passes"] == 4 else "the smoother stops early"
        for k in range(rx.NQ if not ch["ill"] else 0):
            v.value(("lowess", cls), k, info["lowess"][k], ch["fit"][k], ch["fit_unit"][k])
        v.value(("filterThreshold", "all"), j, info["filterThreshold"], mpf_of(c["cut"][j]), mpf_of(c["unit"][j]))
        v.value(("theta", "all"), j, info["filterTheta"], mpf_of(c["theta"][j]), mpf_of(c["theta_unit"][j]))
    # the NA pattern of padj: the rows filter j keeps, under one of its readings, that have a p-value
    got = ~np.isnan(padj)
    has_p = ~np.isnan(p)
    sets = [np.array(s) for s in rx.pass_sets(bm, c, j)]
    match = [s for s in sets if np.array_equal(got, s & has_p)]
    if not match:
        v.violations.append(("padj NA pattern", j, int(got.sum()), [int((s & has_p).sum()) for s in sets]))
    else:
        keep = match[-1]
        judge_bh(v, "padj", np.where(keep, p, np.nan), padj)
    return v


def judge_cooks(case, p_out, nout):
    v = Verdict()
    want = rx.cooks_filter(case["counts"].tolist(), case["group"], case["maxCooks"], case["argmax"], case["pvalue"], case["cutoff"])
    bad = np.flatnonzero(~same_bits(p_out, np.array(want["p"])))
    for i in bad[:5]:
        v.violations.append(("cooks pvalue", int(i), float(p_out[i]), want["p"][i]))
    if int(nout) != sum(want["outlier"]):
        v.violations.append(("cooks count", 0, int(nout), sum(want["outlier"])))
    v.stats = dict(outliers=sum(want["outlier"]), larger=want["larger"])
    return v


def judge_ihw(case, group, weight, wp, wpadj, sample=4000):
    """group where log|avDist| is more than GROUP_ULPS from a break (else excused, counted); weight and weighted_pvalue in units, from
    the groups the candidate itself reported; weighted_padj the IEEE BH sequence over the weighted_pvalue it reported"""
    v = Verdict()
    n = len(group)
    cls = case["name"]
    want_g, dist = twin_of(("ihw groups", case["name"]), lambda: rx.ihw_groups(case["avDist"], case["breaks"]))
    diff = np.flatnonzero(np.asarray(group) != np.array(want_g))
    st = v.stats = dict(group_near=sum(1 for d in dist if d <= GROUP_ULPS), group_excused=[])
    for i in diff:
        if dist[i] <= GROUP_ULPS:
            st["group_excused"].append((int(i), dist[i]))
        elif len(v.violations) < 10:
            v.violations.append(("group", int(i), int(group[i]), want_g[i]))
    wt, wu, mean = rx.ihw_weights([int(g) for g in group], case["weights"], case["pvalue"])
    rows = range(n) if n <= sample else sorted(set(range(0, n, n // sample)) | set(range(300)) | set(range(n - 300, n)))
    pv = case["pvalue"]
    with mp.workdps(rx.DPS):
        seen = {}
        for i in rows:
            if wt[i] is None:
                v.value(("weight", cls), i, weight[i], math.nan, 0)
                v.value(("weighted_pvalue", cls), i, wp[i], math.nan, 0)
                continue
            if wt[i] not in seen:
                seen[wt[i]] = (mpf_of(wt[i]), mpf_of(wu[i]))
            w, u = seen[wt[i]]
            v.value(("weight", cls), i, weight[i], w if w != 0 else 0.0, u)
            pi = float(pv[i])
            if math.isnan(pi) or w == 0:
                v.value(("weighted_pvalue", cls), i, wp[i], math.nan if math.isnan(pi) or pi == 0 else math.inf, 0)
            elif pi == 0:
                v.value(("weighted_pvalue", cls), i, wp[i], 0.0, 0)
            else:
                q = mp.mpf(pi) / w
                v.value(("weighted_pvalue", cls), i, wp[i], q, q * (n + 2) / 2 ** 53)
    if n > sample:   # every row: one IEEE division of p by the weight reported
        with np.errstate(all="ignore"):
            bad = np.flatnonzero(~same_bits(wp, np.asarray(pv) / np.asarray(weight)))
        for i in bad[:5]:
            v.violations.append(("weighted_pvalue != p / weight", int(i), float(wp[i]), float(pv[i] / weight[i])))
    judge_bh(v, "weighted_padj", np.asarray(wp), np.asarray(wpadj))
    return v


def rejected(verdict, bound=SEPARATION):
    return bool(verdict.violations) or any(w > bound for w, _ in verdict.worst().values())


def caps_met(case_name, v, n=None):
    st = v.stats
    if "index_excused" in st:
        assert st["index_excused"] <= NEAR_CAP * st["index_decisions"], (case_name, st)
    if "group_excused" in st:
        assert len(st["group_excused"]) <= NEAR_CAP * n, (case_name, st["group_excused"])


# ---------------------------------------------------------------------------------------------------------------------------
# the yardstick's engine (tests/test_gpu_results.py has the device's)
# ---------------------------------------------------------------------------------------------------------------------------
class YardEngine:
    def __init__(self, oracle):
        self.oracle = oracle

    def filtering(self, bm, p, alpha):
        return yard.independent_filtering(bm, p, alpha)

    def cooks(self, case, pvalue=None):
        pv = case["pvalue"] if pvalue is None else pvalue
        return yard.cooks_filter(pv, case["maxCooks"], case["argmax"], lambda idx: case["counts"][idx], case["group"], cutoff=case["cutoff"])

    def bh(self, p):
        return self.oracle.bh_adjust(p)

    def ihw(self, av, pv, breaks, w):
        return self.oracle.ihw_apply(av, pv, breaks, w)


def run_chain(engine, fit, group, counts):
    """Cook's filter, independent filtering, IHW with seven made-up groups on one fit's own columns; each stage judged on what it was
    really given.  Returns {stage: Verdict}."""
    m, p, applies = rx.design(group)
    n = len(fit["pvalue"])
    ck = dict(name="chain", group=group, counts=counts, argmax=np.asarray(fit["cooksArgmax"]), maxCooks=np.asarray(fit["maxCooks"], dtype=np.float64),
              pvalue=np.asarray(fit["pvalue"], dtype=np.float64), cutoff=float(rx.qf99(p, m - p)))
    pv, nout = engine.cooks(ck)
    out = dict(cooks=judge_cooks(ck, pv, nout))
    fc = dict(name="chain", baseMean=np.asarray(fit["baseMean"], dtype=np.float64), pvalue=np.asarray(pv), alpha=0.1)
    padj, info = engine.filtering(fc["baseMean"], fc["pvalue"], 0.1)
    out["filtering"] = judge_filtering(fc, padj, info)
    breaks, w = ri.chain_ihw_tables()
    ic = dict(name="chain", breaks=breaks, weights=w, avDist=ri.chain_avdist(n), pvalue=np.asarray(pv))
    out["ihw"] = judge_ihw(ic, *engine.ihw(ic["avDist"], ic["pvalue"], breaks, w))
    out["facts"] = dict(outliers=int(nout), na_padj=int(np.isnan(padj).sum()), index=int(info["index"]))
    return out


# ---------------------------------------------------------------------------------------------------------------------------
# the inputs hold what they were built for
# ---------------------------------------------------------------------------------------------------------------------------
def test_planted_edges_are_present():
    """the BH edge: on the `edge` cases the IEEE sequence and the exact comparison part on several decisions, and some planted product
    equals alpha exactly; ties, p = 0, p = 1, NA p and zero baseMean are there; the integer-h sizes have bands; the threshold
    profiles are the ones the names say"""
    for name, least in (("n63-edge", 1), ("n64-integer-edge-a05", 1), ("n4097-edge", 5)):
        case = ri.if_case(name)
        c, rd = if_twin(case)
        assert sum(r["disagree"] for r in rd) >= least, (name, sum(r["disagree"] for r in rd))
        assert len(case["planted"]) >= 3
    case = ri.if_case("n4097-edge")
    a = case["alpha"]
    assert sum(1 for row, r, f, m, _ in case["planted"] if (m / r) * case["pvalue"][row] == a) >= 3
    t = ri.if_case("n4097-ties")["pvalue"]
    assert (t == 0).sum() > 64 and (t == 0.015625).sum() > 1024 - 70 and (t == 1).sum() and np.isnan(t).sum()
    z = ri.if_case("n1023-zeros-na")
    assert ((z["baseMean"] == 0) & ~np.isnan(z["pvalue"])).sum() and (np.isnan(z["pvalue"]) & (z["baseMean"] >= np.quantile(z["baseMean"], 0.97))).sum()
    for name in ("n981-integer-h", "n1961-integer-h", "n4901-integer-h-a05"):
        c, _ = if_twin(ri.if_case(name))
        assert all(c["near_int"]) and all(h.denominator == 1 for h in c["h"]) and sum(1 for b in c["band"] if b) >= 3
        assert max(len(b) for b in c["band"]) == 1
    assert float(if_twin(ri.if_case("n1024-lower-under"))[0]["lower"]) < 0.95 < float(if_twin(ri.if_case("n1025-lower-over"))[0]["lower"])
    assert if_twin(ri.if_case("n2049-lower-one"))[0]["lower"] == 1
    prof = lambda nm: [r["ieee"][-1] for r in if_twin(ri.if_case(nm))[1]]
    assert prof("n1023-max10") == [0] * 30 + [10] * 20 and prof("n1023-max11") == [0] * 30 + [11] * 20 and prof("n1023-plateau") == [0] * 30 + [12] * 20
    assert prof("n1023-constant11") == [11] * 50 and prof("n1023-all-zero") == [0] * 50 and prof("n1023-single-point") == [0] * 49 + [11]
    ab = ri.if_case("n1023-all-below")
    assert np.nanmax(ab["pvalue"]) < ab["alpha"]
    for K in (1024, 1025, 2048):
        e = ri.if_case(f"n3079-exit-{K}")
        ps = np.sort(e["pvalue"])
        assert ps[K - 1] < e["alpha"] == ps[K]
    for name in ri.COOKS_DESIGNS:
        ck = ri.cooks_case(name)
        want = rx.cooks_filter(ck["counts"].tolist(), ck["group"], ck["maxCooks"], ck["argmax"], ck["pvalue"], ck["cutoff"])
        if ck["p"] == 2 and ck["applies"]:
            assert {2, 3} <= set(x for x in want["larger"] if x is not None)
            flagged = ck["counts"][np.arange(ri.COOKS_N), ck["argmax"]]
            assert ((ck["counts"] == flagged[:, None]).sum(1) >= 2).any()
        assert want["applies"] == (name != "S4-0011")
    for name in ri.IHW_CASES[1:-1]:
        _, dist = rx.ihw_groups(ri.ihw_case(name)["avDist"], ri.ihw_case(name)["breaks"])
        assert sum(1 for d in dist if d <= 1.0) >= 2, name


def test_f_quantile_of_the_wrapper_on_record():
    """scipy.stats.f.ppf, which deseq2wrap.py hands to the Cook's filter, against qf(.99, p, m - p) at 50 digits: within a few ulp, so
    only a maxCooks within that of the cutoff could be flagged differently from R"""
    from scipy import stats
    for S in (3, 5, 8, 64):
        p = 1 if S == 3 else 2
        d = rx.ulps_from_qf(stats.f.ppf(0.99, p, S - p), p, S - p)
        print(f"qf(.99, {p}, {S - p}) = {float(rx.qf99(p, S - p))!r}: scipy is {d:.2f} ulp away")
        assert d < 64


# ---------------------------------------------------------------------------------------------------------------------------
# the yardstick under the judge
# ---------------------------------------------------------------------------------------------------------------------------
def report(tag, v):
    for k, (w, n) in sorted(v.worst().items()):
        print(f"{tag} | {k[0]} | {k[1]}: n={n} worst {w:.3g} units")
    print(f"{tag} | stats {getattr(v, 'stats', {})}")


@pytest.mark.parametrize("name", ri.IF_CASES)
def test_yardstick_independent_filtering(name):
    case = ri.if_case(name)
    padj, info = yard.independent_filtering(case["baseMean"], case["pvalue"], case["alpha"])
    v = judge_filtering(case, padj, info)
    report(name, v)
    assert not v.violations, v.violations[:10]
    assert not rejected(v), v.worst()
    caps_met(name, v)


@pytest.mark.parametrize("name", list(ri.COOKS_DESIGNS))
def test_yardstick_cooks_filter(oracle, name):
    case = ri.cooks_case(name)
    v = judge_cooks(case, *YardEngine(oracle).cooks(case))
    assert not v.violations, v.violations


@pytest.mark.parametrize("name", ri.IHW_CASES)
def test_yardstick_ihw_and_bh(oracle, name):
    case = ri.ihw_case(name)
    v = judge_ihw(case, *oracle.ihw_apply(case["avDist"], case["pvalue"], case["breaks"], case["weights"]))
    report(name, v)
    assert not v.violations, v.violations[:10]
    assert not rejected(v), v.worst()
    caps_met(name, v, len(case["avDist"]))
    b = Verdict()
    judge_bh(b, "bh_adjust", case["pvalue"], oracle.bh_adjust(case["pvalue"]))
    assert not b.violations, b.violations


def test_yardstick_chain(oracle):
    import wald_inputs as wi
    from test_wald_twin import columns
    case = wi.make_case("S8-4v4")
    fit = columns(oracle.nbglm_fit(case["counts"], case["nf"], case["group"], **case["opts"]))
    out = run_chain(YardEngine(oracle), fit, case["group"], case["counts"])
    for stage in ("cooks", "filtering", "ihw"):
        report("chain " + stage, out[stage])
        assert not out[stage].violations, (stage, out[stage].violations[:10])
        assert not rejected(out[stage]), (stage, out[stage].worst())
    print(out["facts"])


# ---------------------------------------------------------------------------------------------------------------------------
# wrong readings: variants of a plain restatement built from the twin's pieces
# ---------------------------------------------------------------------------------------------------------------------------
def plain_filtering(case, wrong=None):
    """independent filtering from the twin's pieces: the exact cuts rounded once, the IEEE BH sequence, lowess at 50 digits rounded
    once.  wrong: one of the readings below."""
    bm, p, alpha = case["baseMean"], case["pvalue"], case["alpha"]
    n = len(bm)
    a = float(alpha)
    has_p = [not math.isnan(v) for v in p]
    if wrong == "lower over rows with a p-value":
        c = dict(rx.cuts(bm))
        sub = rx.cuts(bm[~np.isnan(p)]) if (~np.isnan(p)).any() else c
        th = [sub["lower"] + k * (sub["upper"] - sub["lower"]) / (rx.NQ - 1) for k in range(rx.NQ)]
        x = sorted(Fraction(float(v)) for v in bm)
        c["theta"] = th
        c["cut"] = [x[int((n - 1) * t)] + ((n - 1) * t - int((n - 1) * t)) * (x[min(int((n - 1) * t) + 1, n - 1)] - x[int((n - 1) * t)]) for t in th]
        c["band"] = [[] for _ in th]
    elif wrong == "quantile type 1":
        c = dict(rx.cuts(bm))
        x = sorted(Fraction(float(v)) for v in bm)
        c["cut"] = [x[max(math.ceil(n * t), 1) - 1] for t in c["theta"]]
        c["band"] = [[] for _ in c["theta"]]
    else:
        c = if_twin(case)[0]
    order = sorted((i for i in range(n) if has_p[i]), key=lambda i: float(p[i]))
    passes = [rx.pass_sets(bm, c, f, gt=(wrong == "filter > cut"))[-1] for f in range(rx.NQ)]
    numRej = []
    for f in range(rx.NQ):
        ps = [float(p[i]) for i in order if passes[f][i]]
        m = sum(passes[f]) if wrong == "m counts NA p-values" else len(ps)
        r = len(ps)
        while r > 0:
            q = (m * ps[r - 1]) / r if wrong == "m p / r" else (m / r) * ps[r - 1]
            if (q <= a if wrong == "padj <= alpha" else q < a):
                break
            r -= 1
        numRej.append(r)
    kw = dict(f=Fraction(2, 3)) if wrong == "lowess f = 2/3" else dict(iters=0) if wrong == "lowess without robustness" else {}
    fit, _, _ = rx.lowess(c["theta"], numRej, **kw)
    with mp.workdps(rx.DPS):
        j = 0
        if (max(numRej) >= 10) if wrong == "< 10 rule" else (max(numRej) > 10):
            pos = list(range(rx.NQ)) if wrong == "residuals over all 50" else [k for k in range(rx.NQ) if numRej[k] > 0]
            thresh = max(fit) - mp.sqrt(mp.fsum((numRej[k] - fit[k]) ** 2 for k in pos) / len(pos))
            above = [k for k in range(rx.NQ) if (numRej[k] >= thresh if wrong == ">= thresh" else numRej[k] > thresh)]
            j = above[0] if above else 0
        info = dict(theta=[float(mpf_of(t)) for t in c["theta"]], numRej=[float(v) for v in numRej], lowess=[float(v) for v in fit], index=j + 1,
                    filterThreshold=float(mpf_of(c["cut"][j])), filterTheta=float(mpf_of(c["theta"][j])))
    keep = np.array(passes[j])
    padj = np.array(rx.final_padj([float(v) for v in p], [bool(k and h) for k, h in zip(keep, has_p)]))
    return padj, info


# reading -> the case it must be rejected on (and the right reading pass)
WRONG_FILTERING = {
    "padj <= alpha": "n4097-edge",
    "m p / r": "n4097-edge",
    "m counts NA p-values": "n4097-edge",
    "filter > cut": "n1023-zeros-na",
    "quantile type 1": "n1023-zeros-na",
    "lower over rows with a p-value": "n1023-zeros-na",
    "lowess f = 2/3": "n981-integer-h",
    "lowess without robustness": "n981-integer-h",
    "residuals over all 50": "n1023-single-point",
    "< 10 rule": "n1023-max10",
}


@pytest.mark.parametrize("wrong", list(WRONG_FILTERING))
def test_judge_rejects_wrong_filtering(wrong):
    case = ri.if_case(WRONG_FILTERING[wrong])
    right = judge_filtering(case, *plain_filtering(case))
    assert not rejected(right), (right.violations[:5], right.worst())
    bad = judge_filtering(case, *plain_filtering(case, wrong))
    assert rejected(bad), wrong


def test_ge_thresh_parts_from_gt_only_on_an_exact_tie():
    """`numRej >= thresh` for `numRej > thresh`: the two part only where thresh equals an integer exactly — the constant profile, whose
    residuals are zero and whose thresh is its own value.  There R's own doubles decide by the last bit of a lowess fit (the judge
    reports the decision with margin 0 and excuses it), and either way the index is 1: with `>=` every point is above and the first
    is taken; with `>` none is and the rule falls back to the first.  On every other case the reading changes nothing.  So this
    reading cannot be told from the right one by any input on which double arithmetic decides; the test asserts exactly that."""
    case = ri.if_case("n1023-constant11")
    _, info = plain_filtering(case)
    ch = rx.choose(if_twin(case)[0]["theta"], [int(v) for v in info["numRej"]])
    ties = [d for d in ch["decisions"] if d[0] == "numRej > thresh" and d[1] < 1e-20]   # zero but for the 50th digit
    assert len(ties) == rx.NQ and ch["index"] == 1
    for name in ri.IF_CASES:
        c = ri.if_case(name)
        assert plain_filtering(c, ">= thresh")[1]["index"] == plain_filtering(c)[1]["index"], name


def plain_cooks(case, wrong=None):
    m, p, applies = rx.design(case["group"])
    out = case["pvalue"].copy()
    nout = 0
    if applies:
        for i in range(len(out)):
            mc = case["maxCooks"][i]
            flag = mc > case["cutoff"] or (wrong == "NaN is an outlier" and math.isnan(mc))
            if flag and p == 2:
                row = case["counts"][i]
                larger = int((row >= row[case["argmax"][i]]).sum()) if wrong == "rescue counts >=" else int((row > row[case["argmax"][i]]).sum())
                flag = not (larger > 3 if wrong == "rescue at > 3" else larger >= 3)
            if flag:
                out[i] = math.nan
                nout += 1
    return out, nout


@pytest.mark.parametrize("wrong", ["rescue at > 3", "rescue counts >=", "NaN is an outlier"])
def test_judge_rejects_wrong_cooks(wrong):
    case = ri.cooks_case("S8-4v4")
    assert not rejected(judge_cooks(case, *plain_cooks(case)))
    assert rejected(judge_cooks(case, *plain_cooks(case, wrong))), wrong


def plain_ihw(case, wrong=None):
    g, _ = rx.ihw_groups(case["avDist"], case["breaks"], left_closed=(wrong == "left-closed intervals"))
    w = case["weights"]
    pv = case["pvalue"]
    n = len(g)
    wt, _, _ = rx.ihw_weights(g, w, pv)
    if wrong == "mean with na.rm":
        have = [Fraction(float(w[k - 1])) for k in g if k != rx.NA_INT]
        mean = sum(have) / len(have)
        wt = [None if k == rx.NA_INT else Fraction(float(w[k - 1])) / mean for k in g]
    with mp.workdps(rx.DPS), np.errstate(all="ignore"):
        weight = np.array([math.nan if t is None else float(mpf_of(t)) for t in wt])
        wp = np.array([math.nan if t is None or math.isnan(pi) else (np.float64(pi) / np.float64(0.0) if t == 0 else float(mp.mpf(float(pi)) / mpf_of(t)))
                       for t, pi in zip(wt, pv)], dtype=np.float64)
    if wrong == "weighted p capped at 1":
        wp = np.minimum(wp, 1.0)
    if wrong == "BH's n counts NA":
        ok = ~np.isnan(wp)
        wpadj = np.full(n, math.nan)
        o = np.argsort(wp[ok], kind="stable")
        q = np.minimum(1.0, np.minimum.accumulate((n / np.arange(ok.sum(), 0, -1) * wp[ok][o][::-1])))[::-1]
        r = np.empty(ok.sum()); r[o] = q
        wpadj[ok] = r
    else:
        wpadj = np.array(rx.bh_ieee([float(x) for x in wp]))
    return np.array(g), weight, wp, wpadj


WRONG_IHW = {"left-closed intervals": "ng7-dirty", "mean with na.rm": "ng7-dirty", "weighted p capped at 1": "ng7-inf", "BH's n counts NA": "ng7-inf"}


@pytest.mark.parametrize("wrong", list(WRONG_IHW))
def test_judge_rejects_wrong_ihw(wrong):
    case = ri.ihw_case(WRONG_IHW[wrong])
    right = judge_ihw(case, *plain_ihw(case))
    assert not rejected(right), (right.violations[:5], right.worst())
    assert rejected(judge_ihw(case, *plain_ihw(case, wrong))), wrong
    if wrong == "left-closed intervals":   # also where the last break is +Inf: log(Inf) lies inside (b, Inf] and outside [b, Inf)
        inf = ri.ihw_case("ng7-inf")
        assert rejected(judge_ihw(inf, *plain_ihw(inf, wrong)))
