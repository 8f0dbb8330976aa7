"""The judge of the Wald stage, and the CPU oracle before it.

`judge(case, outputs)` holds one fit's Wald columns to tests/wald_twin.py (50 digits): the IRLS's step count and iterate against the
replayed recursion, and — at the REPORTED dispersion, intercept and fold change — both standard errors, stat (bit for bit the quotient
of its two reported operands), p, the largest Cook's distance and its position.  Errors are counted in the units of the issue that
introduced this file (wald_twin.closed_forms: u kappa for a standard error, u max(1, |beta|) for a coefficient, a condition-aware unit
for Cook's distance, u relative for p), per stratum (quantity, row class).

Here the judge runs on oracle.nbglm_fit.  Integer and bit-exact columns must hold on every row; every error must stay under
SEPARATION units — not an accuracy claim: another formula shows as 1e6 units or more, the oracle's arithmetic as a few, and 64 lies
between.  The conditions tests/wald_inputs.py is built to meet are asserted, and six wrong implementations are each shown to be
rejected.  tests/test_gpu_wald.py applies the same judge to the device.
"""
import math
import time

import mpmath as mp
import numpy as np
import pytest

import wald_inputs as wi
import wald_twin as wt

SEPARATION = 64.0      # units: between "another formula" (>= 1e6) and "double arithmetic" (a few)
NEAR_TOL = 1e-3        # a conv_test within this (relative) of betaTol may fall either way in double arithmetic
NEAR_CAP = 0.01        # ... in at most this share of a case's rows
BETA_TOL = 1e-8
SMALL_STRATUM = 20     # fewer rows than this: pooled with the same class of the other cases
P_CUTOFF = 37.5193     # R's pnorm: 2 Phi(-|z|) is 0 from here on
CLASSES = ["betaIter <= 5", "betaIter 6-19", "betaIter 20-99", "optim", "some mu floored", "alpha >= 1"]

_REPLAY, _CLOSED = {}, {}


def columns(out):
    """The oracle's column names -> the library's."""
    o = dict(out)
    for a, b in (("beta0", "intercept"), ("se0", "interceptSE"), ("beta1", "log2FoldChange"), ("se1", "lfcSE")):
        if b not in o and a in o:
            o[b] = o[a]
    return o


def _bits(x):
    return np.ascontiguousarray(x, dtype=np.float64).view(np.uint64)


def same_bits(a, b):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return (_bits(a) == _bits(b)) | (np.isnan(a) & np.isnan(b))


def _key(case, i):
    return (case["group"].tobytes(), case["counts"][i].tobytes(), case["nf"][i].tobytes())


def replay_of(case, i, alpha, extra=0):
    k = _key(case, i) + (float(alpha).hex(), extra)
    if k not in _REPLAY:
        _REPLAY[k] = wt.replay(case["counts"][i], case["nf"][i], case["group"], alpha, extra=extra)
    return _REPLAY[k]


def closed_of(case, i, alpha, b0, b1):
    k = _key(case, i) + (float(alpha).hex(), float(b0).hex(), float(b1).hex())
    if k not in _CLOSED:
        _CLOSED[k] = wt.closed_forms(case["counts"][i], case["nf"][i], case["group"], alpha, b0, b1)
    return _CLOSED[k]


def near_tolerance(c):
    return c is not None and abs(c / BETA_TOL - 1) < NEAR_TOL


def judge(case, outputs, rows=None):
    """Every row of `rows` (default: all) of one fit against the twin.  Returns
      errors      {(quantity, class): [(error in units, row), ...]}
      violations  [(row, what, detail)]: step counts, bit-exact stat, arg-max, all-zero rows, non-finite values
      near        rows whose step count differs from the twin's by one at a conv_test within NEAR_TOL of betaTol (allowed, capped)
      stats       what the twin saw: rows with an exact arg-max tie, with a floored mu at the final beta, per step class, with a
                  conv_test near the tolerance anywhere in the trace, not converged (betaConv == 0: nothing but the step count is judged)."""
    with mp.workdps(wt.DPS):
        return _judge(case, columns(outputs), range(len(case["counts"])) if rows is None else [int(r) for r in rows])


def _rel(got, ref, unit):
    if not math.isfinite(got):
        return math.inf
    if ref == 0:
        return 0.0 if got == 0 else math.inf
    return float(abs(mp.mpf(float(got)) - ref) / (abs(ref) * unit))


def _judge(case, o, rows):
    errors, violations = {}, []
    stats = dict(rows=len(rows), tie=0, floored=0, it_20_99=0, it_100=0, near_trace=0, not_converged=0, mismatched=0)
    near = 0
    two = case["two_groups"]
    counts = case["counts"]
    with np.errstate(invalid="ignore", divide="ignore"):
        quotient = (o["log2FoldChange"] if two else o["intercept"]) / (o["lfcSE"] if two else o["interceptSE"])
    stat_ok = same_bits(o["stat"], quotient)

    def add(q, classes, e, i):
        for c in classes:
            errors.setdefault((q, c), []).append((e, i))

    for i in rows:
        if counts[i].sum() == 0:
            nan_cols = ["log2FoldChange", "lfcSE", "stat", "pvalue", "intercept", "interceptSE", "maxCooks"]
            bad = [k for k in nan_cols if not np.isnan(o[k][i])] + [k for k, v in (("betaIter", 0), ("betaConv", 0), ("cooksArgmax", -1)) if o[k][i] != v]
            if bad:
                violations.append((i, "all-zero row", bad))
            continue
        if not stat_ok[i]:
            violations.append((i, "stat is not the quotient of its reported operands", (float(o["stat"][i]).hex(), float(quotient[i]).hex())))
        alpha, b0, b1 = float(o["dispersion"][i]), float(o["intercept"][i]), float(o["log2FoldChange"][i])
        it, conv = int(o["betaIter"][i]), int(o["betaConv"][i])
        if not (math.isfinite(alpha) and alpha > 0 and math.isfinite(b0)):
            violations.append((i, "dispersion / intercept not finite", (alpha, b0)))
            continue
        if not two:
            cf = closed_of(case, i, alpha, b0, 0.0)
            cls = ["betaIter <= 5"] + (["alpha >= 1"] if alpha >= 1 else [])
            if it != 1 or conv != 1 or not np.isnan(o["log2FoldChange"][i]) or not np.isnan(o["lfcSE"][i]) or not np.isnan(o["maxCooks"][i]) or o["cooksArgmax"][i] != -1:
                violations.append((i, "design ~1: betaIter, betaConv 1, lfc / lfcSE / maxCooks NaN, arg-max -1", (it, conv)))
            add("intercept", cls, float(abs(mp.mpf(b0) - cf["intercept"]) / cf["beta_unit"]), i)
            add("interceptSE", cls, _rel(o["interceptSE"][i], cf["interceptSE"], cf["se_unit"]), i)
            _judge_p(o, i, cls, add, violations)
            continue
        if not math.isfinite(b1):
            violations.append((i, "log2FoldChange not finite", b1))
            continue
        rp = replay_of(case, i, alpha)
        stop = rp["stop"]
        stats["it_20_99"] += 20 <= stop <= 99
        stats["it_100"] += stop >= 100
        stats["near_trace"] += any(near_tolerance(c) for c in rp["conv"][2:stop + 1])
        cls = ["betaIter <= 5" if it <= 5 else "betaIter 6-19" if it <= 19 else "betaIter 20-99" if it <= 99 else "optim"]
        if alpha >= 1:
            cls.append("alpha >= 1")
        if it != stop:
            stats["mismatched"] += 1
            if it == stop + 1:
                rp = replay_of(case, i, alpha, extra=1)  # the same trace, one tick beyond its stop
            at = min(it, stop)
            if abs(it - stop) == 1 and 2 <= at < len(rp["conv"]) and near_tolerance(rp["conv"][at]):
                near += 1
            else:
                violations.append((i, "betaIter", (it, stop, [float(c) for c in rp["conv"][max(1, at - 1):at + 2]])))
                continue
        if conv != 1:
            stats["not_converged"] += 1
            continue
        cf = closed_of(case, i, alpha, b0, b1)
        stats["tie"] += cf["tie"]
        stats["floored"] += cf["floored"] > 0
        if cf["floored"]:
            cls.append("some mu floored")
        if it < 100:
            if it >= len(rp["betas"]):
                violations.append((i, "betaIter beyond the replayed trace", (it, stop)))
                continue
            t0, t1 = (v / mp.log(2) for v in rp["betas"][it])
            unit = wt.U * max(mp.mpf(1), abs(t0), abs(t1))
            add("beta", cls, float(max(abs(mp.mpf(b0) - t0), abs(mp.mpf(b1) - t1)) / unit), i)
        add("lfcSE", cls, _rel(o["lfcSE"][i], cf["lfcSE"], cf["se_unit"]), i)
        add("interceptSE", cls, _rel(o["interceptSE"][i], cf["interceptSE"], cf["se_unit"]), i)
        _judge_p(o, i, cls, add, violations)
        mc, am = float(o["maxCooks"][i]), int(o["cooksArgmax"][i])
        if cf["cooks"] is None:
            if not math.isnan(mc) or am != -1:
                violations.append((i, "no cell of 3: maxCooks must be NaN and the arg-max -1", (mc, am)))
            continue
        j = cf["maxCooksAt"]
        unit = cf["cooks_unit"][j]
        if unit is None:  # y == mu_f exactly at the maximum: every distance of the counted cells is 0
            if mc != 0.0:
                violations.append((i, "maxCooks", (mc, 0.0)))
        else:
            add("maxCooks", cls, _rel(mc, cf["maxCooks"], unit), i)
        first = cf["cooksArgmax"]
        if am != first:
            ck = cf["cooks"]
            u1 = cf["cooks_unit"][first]
            close = 0 <= am < case["S"] and ck[am] != ck[first] and u1 is not None and abs(ck[am] - ck[first]) <= ck[first] * u1
            if not close:
                violations.append((i, "cooksArgmax", (am, first, "exact tie" if 0 <= am < case["S"] and ck[am] == ck[first] else "not within a unit")))
    return dict(errors=errors, violations=violations, near=near, stats=stats)


def _judge_p(o, i, cls, add, violations):
    st, p = float(o["stat"][i]), float(o["pvalue"][i])
    if not math.isfinite(st):
        violations.append((i, "stat not finite", st))
    elif abs(st) >= P_CUTOFF:
        if p != 0.0:
            violations.append((i, "p beyond the cutoff must be 0", (st, p)))
    else:
        add("pvalue", cls, _rel(p, wt.p_two_sided(st), wt.U), i)


def pooled(results, partition=None):
    """{case: judge result} -> {(case or "pooled", quantity, class): (worst, rows, where)}: a stratum of fewer than SMALL_STRATUM rows
    joins the same stratum of the other cases.  `partition` (a set of (case, quantity, class) that stand alone), when given, is used
    instead of the row counts, so that two fits of the same inputs are divided the same way; it is returned as the second value."""
    own = set(partition) if partition is not None else {(c, q, k) for c, r in results.items() for (q, k), v in r["errors"].items() if len(v) >= SMALL_STRATUM}
    acc = {}
    for c, r in results.items():
        for (q, k), v in r["errors"].items():
            acc.setdefault((c if (c, q, k) in own else "pooled", q, k), []).extend((e, (c, i)) for e, i in v)
    return {key: (max(v)[0], len(v), max(v)[1]) for key, v in acc.items()}, own


def rejected(res, bound=SEPARATION):
    """What a wrong implementation must bring about: a violation, or an error beyond the separation."""
    return bool(res["violations"]) or any(e > bound for v in res["errors"].values() for e, _ in v)


# ---------------------------------------------------------------------------------------------------------------------------
# the oracle under the judge
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def oracle():
    from oracle import oracle as o
    o.build()
    return o


_FITS = {}


def oracle_fit(oracle, name):
    if name not in _FITS:
        case = wi.make_case(name)
        t0 = time.perf_counter()
        ref = columns(oracle.nbglm_fit(case["counts"], case["nf"], case["group"], **case["opts"]))
        res = judge(case, ref)
        print(f"{name}: judged {len(case['counts'])} rows in {time.perf_counter() - t0:.1f} s; {res['stats']}")
        _FITS[name] = (case, ref, res)
    return _FITS[name]


@pytest.mark.parametrize("name", list(wi.DESIGNS))
def test_oracle_against_twin(oracle, name):
    """The oracle's Wald columns, every row: step counts equal to the replay's (not one row at the tolerance stops elsewhere: the seeds
    of wald_inputs are chosen so), stat bit-exact, the arg-max the twin's first maximum, every error below SEPARATION units — and the
    conditions the inputs are built to meet."""
    case, ref, res = oracle_fit(oracle, name)
    for (q, k), v in sorted(res["errors"].items()):
        print(f"  {q} | {k}: n={len(v)} worst {max(v)[0]:.3g} units (row {max(v)[1]})")
    assert not res["violations"], res["violations"][:10]
    assert res["near"] == 0 and res["stats"]["mismatched"] == 0
    worst = {k: max(v) for k, v in res["errors"].items()}
    assert all(e < SEPARATION for e, _ in worst.values()), {k: w for k, w in worst.items() if not w[0] < SEPARATION}
    st, n = res["stats"], len(case["counts"])
    assert st["near_trace"] <= NEAR_CAP * n, st
    if case["two_groups"]:
        assert st["floored"] >= 20 and st["it_20_99"] >= 3 and st["it_100"] >= 3, st
        if case["S"] >= 5:
            assert st["tie"] >= 8, st  # (2 v 2 has no Cook's distances: the arg-max is -1 by definition)
        else:
            assert np.isnan(ref["maxCooks"]).all() and (ref["cooksArgmax"] == -1).all()
    # the planted rows do what they were planted for
    p = case["planted"]
    assert (ref["allZero"][p["zero"]] == 1).all()
    if case["two_groups"]:
        assert (ref["betaIter"][p["bzero"]] <= 5).all() and (ref["betaIter"][p["huge"]] == 100).sum() >= 3


def test_pooled_strata_of_the_oracle(oracle):
    """Strata too small to stand alone in a case, pooled over the cases: the same separation."""
    strata, _ = pooled({name: oracle_fit(oracle, name)[2] for name in wi.DESIGNS})
    small = {k: v for k, v in strata.items() if k[0] == "pooled"}
    for k, (w, n, at) in sorted(small.items()):
        print(f"  {k}: n={n} worst {w:.3g} units at {at}")
    assert all(w < SEPARATION for w, _, _ in strata.values()), {k: v for k, v in strata.items() if not v[0] < SEPARATION}
    for q in ("beta", "lfcSE", "interceptSE", "pvalue", "maxCooks"):
        for c in CLASSES:
            if (q, c) != ("beta", "optim"):  # (the optimiser's result is no iterate of the recursion: judged by its closed forms only)
                assert any(k[1] == q and k[2] == c for k in strata), (q, c)  # no other stratum is empty


# ---------------------------------------------------------------------------------------------------------------------------
# the judge can fail: six wrong implementations
# ---------------------------------------------------------------------------------------------------------------------------
LOG2E = 1.0 / math.log(2.0)
LAMBDA = 1e-6 / (math.log(2.0) * math.log(2.0))


def _trimmed(vals, lo, wrong_end):
    """mean(vals, trim) by ranks, equal values ranked by index.  wrong_end: at the LOW end the highest index among equals goes first
    (the high end still drops the highest index first) — in a run of equal values that reaches from one end to the other the same
    elements are then dropped twice, and too many stay."""
    n = len(vals)
    idx = list(range(n))
    low = sorted(idx, key=lambda j: (vals[j], -j if wrong_end else j))[:lo]
    high = sorted(idx, key=lambda j: (vals[j], j))[n - lo:]
    return sum(vals[j] for j in idx if j not in low and j not in high) / (n - 2 * lo)


def double_wald(case, o, i, floor=True, sandwich=True, wrong_trim=False):
    """One row's standard errors and Cook's distances in double arithmetic at the reported parameters, with a switch for each of the
    wrong formulas below (all switches off: the right formulas, in the same arithmetic, so that only the switch makes the difference)."""
    y, nf, g = case["counts"][i].astype(float), case["nf"][i], case["group"]
    alpha = float(o["dispersion"][i])
    eta = (o["intercept"][i] + o["log2FoldChange"][i] * g) * math.log(2.0)
    muf = nf * np.exp(eta)
    mu = np.maximum(muf, 0.5) if floor else muf
    w = mu / (1 + alpha * mu)
    wA, wB = w[g == 0].sum(), w[g == 1].sum()
    m00, m01, m11 = wA + wB + LAMBDA, wB, wB + LAMBDA
    det = m00 * m11 - m01 * m01
    i00, i01, i11 = m11 / det, -m01 / det, m00 / det
    if sandwich:
        a00, a01, a11 = wA + wB, wB, wB
        t00, t01, t10, t11 = i00 * a00 + i01 * a01, i00 * a01 + i01 * a11, i01 * a00 + i11 * a01, i01 * a01 + i11 * a11
        v0, v1 = t00 * i00 + t01 * i01, t10 * i01 + t11 * i11
    else:
        v0, v1 = i00, i11
    res = dict(interceptSE=LOG2E * math.sqrt(v0), lfcSE=LOG2E * math.sqrt(v1), maxCooks=math.nan, cooksArgmax=-1, cooks=None)
    size = [(g == 0).sum(), (g == 1).sum()]
    if max(size) < 3:
        return res
    q = y / nf
    m = q.mean()
    v = -math.inf
    for c in (0, 1):
        if size[c] < 3:
            continue
        cell = list(q[g == c])
        lo, scale = wt.trim_class(len(cell))
        cm = _trimmed(cell, lo, wrong_trim)
        v = max(v, scale * _trimmed([(x - cm) ** 2 for x in cell], lo, wrong_trim))
    arob = max((v - m) / (m * m), 0.04)
    h = w * np.where(g == 1, i00 + 2 * i01 + i11, i00)
    ck = (y - muf) ** 2 / (muf + arob * muf * muf) / 2 * h / (1 - h) ** 2
    counted = np.array([size[c] >= 3 for c in g])
    res.update(maxCooks=float(ck[counted].max()), cooksArgmax=int(np.argmax(ck)), cooks=ck)
    return res


def _sample(case, kinds, extra=24):
    p = case["planted"]
    free = np.arange(int(p["zero"][-1]) + 1, int(p["copies"][1][0]))
    return np.unique(np.concatenate([p[k] for k in kinds if k in p] + [free[:extra]]))


def _with(oracle, ref, rows, **cols):
    """A copy of the oracle's columns with `cols` replaced on `rows`; stat and p follow a changed lfcSE, as they would in a fit."""
    o = {k: (np.array(v, copy=True) if isinstance(v, np.ndarray) else v) for k, v in ref.items()}
    for k, v in cols.items():
        o[k][rows] = v
    if "lfcSE" in cols:
        o["stat"][rows] = o["log2FoldChange"][rows] / o["lfcSE"][rows]
        o["pvalue"][rows] = oracle.pnorm_two_sided(o["stat"][rows])
    return o


def _flagged(res, rows):
    bad = {i for i, _, _ in res["violations"]} | {i for v in res["errors"].values() for e, i in v if e > SEPARATION}
    return len(bad & set(int(r) for r in rows))


@pytest.mark.parametrize("name", wi.CONDITION_CASES)
def test_judge_rejects_wrong_standard_errors(oracle, name):
    """(a) lfcSE from M^-1 instead of the sandwich M^-1 X'WX M^-1 — every ~condition case, every row; (b) weights without the 0.5 floor
    on mu — every ~condition case, on the rows with a floored mu.  First: the right formulas in the same double arithmetic pass."""
    case, ref, _ = oracle_fit(oracle, name)
    rows = _sample(case, ("slow", "huge", "tie"))
    rows = rows[ref["betaConv"][rows] == 1]
    right = [double_wald(case, ref, i) for i in rows]
    cols = lambda rs, ks: {k: np.array([r[k] for r in rs]) for k in ks}
    keys = ("lfcSE", "interceptSE", "maxCooks", "cooksArgmax")
    assert not rejected(judge(case, _with(oracle, ref, rows, **cols(right, keys)), rows))
    a = judge(case, _with(oracle, ref, rows, **cols([double_wald(case, ref, i, sandwich=False) for i in rows], ("lfcSE",))), rows)
    assert not a["violations"] and _flagged(a, rows) == len(rows), (name, _flagged(a, rows), len(rows))
    with mp.workdps(wt.DPS):
        fl = np.array([closed_of(case, i, ref["dispersion"][i], ref["intercept"][i], ref["log2FoldChange"][i])["floored"] > 0 for i in rows])
    assert fl.sum() >= 10
    b = judge(case, _with(oracle, ref, rows[fl], **cols([double_wald(case, ref, i, floor=False) for i in rows[fl]], keys)), rows)
    assert _flagged(b, rows[fl]) == fl.sum() and _flagged(b, rows[~fl]) == 0, (name, _flagged(b, rows[fl]), fl.sum())


@pytest.mark.parametrize("name", [n for n in wi.CONDITION_CASES if wi.DESIGNS[n][0] >= 5])
def test_judge_rejects_wrong_ties(oracle, name):
    """(c) a trimmed mean that drops the highest index among equal values at the low end: it can show only where a run of equal values
    reaches from the low end of a cell to its high end — the planted rows whose cells are constant — in every case with Cook's
    distances (S >= 5); (d) the LAST of the tied maxima as cooksArgmax: every row with an exact tie, the same cases."""
    case, ref, _ = oracle_fit(oracle, name)
    tie = case["planted"]["tie"]
    g = case["group"]
    flat = np.array([i for i in tie if all(len(set(case["counts"][i][g == c])) == 1 for c in (0, 1))])
    assert len(flat) >= 4
    wrong = [double_wald(case, ref, i, wrong_trim=True) for i in flat]
    c = judge(case, _with(oracle, ref, flat, maxCooks=np.array([r["maxCooks"] for r in wrong])), tie)
    assert _flagged(c, flat) == len(flat), (name, c["violations"], _flagged(c, flat))
    right = [double_wald(case, ref, i) for i in tie]
    last = np.array([int(np.flatnonzero(r["cooks"] == r["cooks"].max())[-1]) for r in right])
    assert (last != ref["cooksArgmax"][tie]).sum() >= 8
    d = judge(case, _with(oracle, ref, tie, cooksArgmax=last), tie)
    assert {i for i, what, _ in d["violations"] if what == "cooksArgmax"} == set(int(i) for i in tie[last != ref["cooksArgmax"][tie]])


@pytest.mark.parametrize("name", wi.CONDITION_CASES)
def test_judge_rejects_an_iterate_taken_one_step_early(oracle, name):
    """(e) beta of step betaIter - 1 reported as the result: every ~condition case, rows that stopped by convergence.  (The last step of a
    converging IRLS still moves beta by far more than a unit: the stop is on the deviance, which is flat to second order.)"""
    case, ref, _ = oracle_fit(oracle, name)
    rows = _sample(case, ("slow", "huge"))
    rows = rows[(ref["betaIter"][rows] < 100) & (ref["betaIter"][rows] >= 3)]
    assert len(rows) >= 20
    b0, b1 = np.empty(len(rows)), np.empty(len(rows))
    for t, i in enumerate(rows):
        it = int(ref["betaIter"][i])
        i0, l1, _ = oracle.irls_trace(case["counts"], case["nf"], case["group"], i, ref["dispersion"][i], steps=it, with_intercept=True)
        # the trace is the fit's (it divides by ln 2 where the fit multiplies by log2 e: two roundings apart at the most)
        assert abs(l1[it - 1] - ref["log2FoldChange"][i]) <= 2 * np.spacing(abs(l1[it - 1]))
        b0[t], b1[t] = i0[it - 2], l1[it - 2]
    e = judge(case, _with(oracle, ref, rows, intercept=b0, log2FoldChange=b1, stat=b1 / ref["lfcSE"][rows]), rows)
    early = {i for v in (e["errors"].get(("beta", c), []) for c in CLASSES) for err, i in v if err > SEPARATION}
    assert early == set(int(i) for i in rows), (name, len(early), len(rows))


@pytest.mark.parametrize("name", list(wi.DESIGNS))
def test_judge_rejects_stat_off_by_one_ulp(oracle, name):
    """(f) every case, ~1 included, every row that is not all zero."""
    case, ref, _ = oracle_fit(oracle, name)
    rows = _sample(case, ("huge", "tie"))
    f = judge(case, _with(oracle, ref, rows, stat=np.nextafter(ref["stat"][rows], np.inf)), rows)
    assert {i for i, what, _ in f["violations"] if what.startswith("stat is not")} == set(int(i) for i in rows)
