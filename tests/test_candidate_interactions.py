"""getCandidateInteractions (chicdiff.R:2068-2163): the C ABI's device join, the binding and the mirror against the literal twin
(tests/candidates_twin.py).  Integer outputs and min_p are compared by equality (min_p through its int64 view, NaN in the same
places); delta, the one value with rounding in it, in units of 2^-52 max(|asinh a|, |asinh b|)."""
import ctypes as C
import functools
import inspect
import json
import os
import re
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import candidates_inputs as ci  # noqa: E402
import candidates_twin as tw  # noqa: E402

SCORE = ci.SCORE
# delta against the twin, in units of 2^-52 max(|asinh a|, |asinh b|) (a relative bound on delta itself would be wrong: the difference
# cancels).  Measured on an MI355X over the reference's regions and the adversarial tables (profiles/r15_candidates_accuracy.json):
# 1.853 units at most — each of the two asinh()s may differ by an ulp between the device's library and the host's libm, as
# test_results_postprocessing.py notes for two libms in general, and the subtraction rounds once more; the row sums are exact on
# both sides.  The bound is twice that figure, rounded up to a whole unit.
DELTA_BOUND_UNITS = 4.0
ACCURACY = {}


@pytest.fixture(scope="module", autouse=True)
def accuracy_record():
    yield
    out = os.environ.get("CHICDIFF_ACCURACY_OUT")   # a directory: keep the figures behind the delta assertions (-> profiles/r15_candidates_accuracy.json)
    if ACCURACY and out:
        os.makedirs(out, exist_ok=True)
        with open(os.path.join(out, "r15_candidates_accuracy.json"), "w") as f:
            json.dump(dict(unit="2^-52 * max(|asinh(mean cond 1)|, |asinh(mean cond 2)|) (merged: max(|col1|, |col2|))",
                           bound_asserted=DELTA_BOUND_UNITS, max_units=max(ACCURACY.values()), cases=ACCURACY), f, indent=1)


# ---- without a GPU --------------------------------------------------------------------------------------------------------------
def test_declared_cited_exported():
    import __graft_entry__ as g
    g.build()
    from chicdiff_amd import hip, pipeline
    hdr = open(os.path.join(ROOT, "include", "chicdiff_hip.h")).read()
    k = hdr.index("int chicdiff_hip_candidate_interactions_dev(")
    comment = hdr[hdr.rindex("/*", 0, k):k]
    assert "2068-2163" in comment and "unpinned" in comment and "NO asinh" in comment
    assert "chicdiff_hip_candidate_interactions_dev" in hip.EXPORTS
    assert hasattr(hip.load_library(), "chicdiff_hip_candidate_interactions_dev")
    assert callable(hip.HipContext.candidate_interactions)
    ref = json.load(open(os.path.join(ROOT, "tests", "golden", "reference_functions.json")))["getCandidateInteractions"]
    sig = inspect.signature(pipeline.getCandidateInteractions)
    assert list(sig.parameters) == [a.replace(".", "_") for a in ref] + ["ctx"]
    d = {k: v.default for k, v in sig.parameters.items()}
    assert (d["pcol"], d["method"], d["minDeltaAsinhScore"], d["pvcut"], d["ctx"]) == ("weighted_padj", "min", 1, 0.05, None)
    mk = open(os.path.join(ROOT, "chicdiff_amd", "csrc", "Makefile")).read()
    assert "candidate_kernels.hip" in re.search(r"^SRCS\s*:=(.*)$", mk, re.M).group(1)


def test_hmp_and_unknown_method_raise_before_a_device_is_needed():
    from chicdiff_amd import pipeline
    with pytest.raises(ValueError, match=r"Unknown method to combine p-values \(should be 'min' or 'hmp'\)"):
        pipeline.getCandidateInteractions(None, None, {}, method="fisher", ctx=None)
    with pytest.raises(ValueError, match=r"harmonicmeanp::p\.hmp"):
        pipeline.getCandidateInteractions(None, None, {}, method="hmp", ctx=None)


@pytest.mark.parametrize("npeaks,nregions,big", [(65, 65, False), (513, 700, False), (300, 700, True)])
def test_twin_equals_brute_force(npeaks, nregions, big):
    case = ci.adversarial_case(npeaks, nregions, 11 * npeaks + nregions, big_bait=big)
    for pvcut, mind in ((0.05, 1.0), (1.0, 0.0)):
        t = tw.candidates_literal(*ci.twin_args(case, case["p"]), SCORE, pvcut, mind)
        b = tw.candidates_brute_force(*ci.twin_args(case, case["p"]), SCORE, pvcut, mind)
        assert len(b) == len(t["groups"]) and (pvcut < 1 or len(b) > 0)
        for x, y in zip(t["groups"], b):
            assert x[0] == y[0] and x[3] == y[3] and x[1] == y[1] and x[2] == y[2]
    if big:
        assert max(len(g[3]) for g in t["groups_all"]) > 64


# ---- on the GPU -----------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def ctx():
    import __graft_entry__ as g
    g.build()
    from chicdiff_amd import hip
    c = hip.HipContext(0)
    yield c
    c.close()


def run_device(ctx, case, p, merged, pvcut, mind, score=SCORE, **kw):
    torch = ctx.torch
    dev = lambda a, dt: torch.from_numpy(np.ascontiguousarray(a, dtype=dt)).to(ctx.device)
    s = case["scores"][:2] if merged else case["scores"]
    nc1 = 1 if merged else s.shape[0] // 2
    return ctx.candidate_interactions(dev(case["baitID"], np.int32), dev(case["minOE"], np.int32), dev(case["maxOE"], np.int32),
                                      dev(p, np.float64), dev(case["peak_baitID"], np.int32), dev(case["peak_oeID"], np.int32),
                                      dev(s, np.float64), nc1, s.shape[0] - nc1, merged, score, pvcut, mind, **kw)


def same_bits(a, b):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    na = np.isnan(a)
    return a.shape == b.shape and np.array_equal(na, np.isnan(b)) and np.array_equal(a[~na].view(np.int64), b[~na].view(np.int64))


def compare(res, twin, label):
    groups = twin["groups"]
    assert res["ngroups"] == len(groups) and res["npairs"] == sum(len(g[3]) for g in groups), (res["ngroups"], len(groups))
    assert np.array_equal(res["group_peak"].cpu().numpy(), np.array([g[0] for g in groups], dtype=np.int32))
    assert np.array_equal(res["group_ptr"].cpu().numpy(), np.concatenate([[0], np.cumsum([len(g[3]) for g in groups])]).astype(np.int64))
    assert np.array_equal(res["pair_row"].cpu().numpy(), np.array([r for g in groups for r in g[3]], dtype=np.int32))
    assert same_bits(res["group_min_p"].cpu().numpy(), [g[1] for g in groups])
    if groups:
        want = np.array([g[2] for g in groups])
        unit = 2.0 ** -52 * np.array([twin["scale"][g[0]] for g in groups])
        dev = np.abs(res["group_delta"].cpu().numpy() - want) / np.where(unit > 0, unit, 1.0)
        ACCURACY[label] = float(dev.max())
        print(f"{label}: delta off by at most {dev.max():.3f} units over {len(groups)} groups")
        assert dev.max() <= DELTA_BOUND_UNITS, (label, float(dev.max()))


@functools.lru_cache(maxsize=None)
def _golden_table():
    return np.load(os.path.join(ROOT, "tests", "golden", "chr19_results.npz"), allow_pickle=True)


@functools.lru_cache(maxsize=None)
def _golden_case():
    return ci.golden_case(_golden_table())


@functools.lru_cache(maxsize=None)
def _golden_twin(pcol, pvcut, mind):
    return tw.candidates_literal(*ci.twin_args(_golden_case(), _golden_table()[pcol]), SCORE, pvcut, mind)


@pytest.mark.gpu
@pytest.mark.parametrize("pcol", ["weighted_padj", "padj"])
@pytest.mark.parametrize("pvcut,mind", [(0.05, 1.0), (1.0, 0.0)])
def test_reference_regions(ctx, pcol, pvcut, mind):
    case, twin = _golden_case(), _golden_twin(pcol, pvcut, mind)
    assert len(twin["groups"]) > 0
    assert any(s and d != d for s, d in zip(twin["selected"], twin["delta"]))          # a selected peak with NA delta
    if pcol == "padj":
        assert sum(g[1] != g[1] for g in twin["groups_all"]) > 0                       # groups whose minimum is NA
    compare(run_device(ctx, case, _golden_table()[pcol], False, pvcut, mind), twin, f"chr19/{pcol}/{pvcut}/{mind}")


@pytest.mark.gpu
@pytest.mark.parametrize("nregions", [1, 2, 65, 700])
@pytest.mark.parametrize("npeaks", [1, 2, 63, 64, 65, 511, 512, 513, 4097])
def test_adversarial(ctx, npeaks, nregions):
    case = ci.adversarial_case(npeaks, nregions, 1000 * npeaks + nregions)
    for pvcut, mind in ((0.05, 1.0), (1.0, 0.0)):
        twin = tw.candidates_literal(*ci.twin_args(case, case["p"]), SCORE, pvcut, mind)
        compare(run_device(ctx, case, case["p"], False, pvcut, mind), twin, f"adv/{npeaks}x{nregions}/{pvcut}/{mind}")


@pytest.mark.gpu
@pytest.mark.parametrize("merged", [False, True])
def test_adversarial_one_bait_with_3000_regions(ctx, merged):
    case = ci.adversarial_case(513, 700, 99, big_bait=True)
    twin = tw.candidates_literal(*ci.twin_args(dict(case, scores=case["scores"][:2]) if merged else case, case["p"], merged), SCORE, 1.0, 0.0)
    assert max(len(g[3]) for g in twin["groups"]) > 64 and len(twin["groups"]) > 50
    compare(run_device(ctx, case, case["p"], merged, 1.0, 0.0), twin, f"adv/big/merged={int(merged)}")


def _stack_case():
    """Two peaks inside 65 identical regions: 130 pairs, more than the binding's first 16 npeaks."""
    return dict(baitID=np.full(65, 1, np.int32), minOE=np.full(65, 5, np.int32), maxOE=np.full(65, 20, np.int32), p=np.full(65, 0.01),
                peak_baitID=np.array([1, 1], np.int32), peak_oeID=np.array([11, 10], np.int32),
                scores=np.array([[50.0, 60.0], [40.0, 70.0], [1.0, 2.0], [2.0, 1.0]]))


@pytest.mark.gpu
def test_capacity(ctx):
    from chicdiff_amd import hip
    torch = ctx.torch
    case = _stack_case()
    twin = tw.candidates_literal(*ci.twin_args(case, case["p"]), SCORE, 0.05, 1.0)
    assert sum(len(g[3]) for g in twin["groups"]) == 130
    buf = torch.full((129,), -1, dtype=torch.int32, device=ctx.device)
    with pytest.raises(hip.ChicdiffHipError, match=r"room for 130 pairs needed, 129 given") as e:
        run_device(ctx, case, case["p"], False, 0.05, 1.0, pair_row=buf)
    assert e.value.need == (2, 130) and bool((buf == -1).all())                       # both counts, no pair
    buf = torch.full((130,), -1, dtype=torch.int32, device=ctx.device)
    exact = run_device(ctx, case, case["p"], False, 0.05, 1.0, pair_row=buf)
    compare(exact, twin, "capacity/exact")
    retried = run_device(ctx, case, case["p"], False, 0.05, 1.0)                        # 16 * 2 < 130: the binding calls twice
    for k in ("group_peak", "group_ptr", "pair_row"):
        assert torch.equal(exact[k], retried[k])
    for k in ("group_min_p", "group_delta"):
        assert same_bits(exact[k].cpu().numpy(), retried[k].cpu().numpy())


@pytest.mark.gpu
def test_refusals_and_empty_outputs(ctx):
    from chicdiff_amd import hip
    base = ci.adversarial_case(65, 65, 5)
    bad = dict(base, minOE=base["minOE"].copy())
    bad["minOE"][3] = bad["maxOE"][3] + 1
    with pytest.raises(hip.ChicdiffHipError, match=r"region row 3 has minOE > maxOE"):
        run_device(ctx, bad, base["p"], False, 0.05, 1.0)
    bad = dict(base, baitID=base["baitID"].copy())
    bad["baitID"][2] = np.iinfo(np.int32).min
    with pytest.raises(hip.ChicdiffHipError, match=r"region row 2 has"):
        run_device(ctx, bad, base["p"], False, 0.05, 1.0)
    bad = dict(base, peak_baitID=base["peak_baitID"].copy(), peak_oeID=base["peak_oeID"].copy(), scores=base["scores"].copy())
    bad["peak_baitID"][4], bad["peak_oeID"][4] = bad["peak_baitID"][1], bad["peak_oeID"][1]
    bad["scores"][:, [1, 4]] = 9.0                                                      # both selected
    with pytest.raises(hip.ChicdiffHipError, match=r"peak row 4 repeats"):
        run_device(ctx, bad, base["p"], False, 0.05, 1.0)
    bad["scores"][:, 4] = 1.0                                                           # an unselected duplicate is no refusal
    run_device(ctx, bad, base["p"], False, 0.05, 1.0)
    with pytest.raises(hip.ChicdiffHipError):                                           # ncols < 2
        run_device(ctx, dict(base, scores=base["scores"][:1]), base["p"], True, 0.05, 1.0)
    with pytest.raises(hip.ChicdiffHipError):                                           # n < 1
        run_device(ctx, dict(base, baitID=base["baitID"][:0], minOE=base["minOE"][:0], maxOE=base["maxOE"][:0]), base["p"][:0], False, 0.05, 1.0)
    # npeaks >= 2^31: refused from the arguments alone (nothing is read)
    t = ctx.torch.zeros(8, dtype=ctx.torch.int64, device=ctx.device)
    ng, npairs = C.c_int64(0), C.c_int64(0)
    rc = ctx.lib.chicdiff_hip_candidate_interactions_dev(ctx.h, *[t.data_ptr()] * 4, 1, *[t.data_ptr()] * 3, 1 << 31, 2, 1, 1, 0, 5.0, 0.05, 1.0, 1,
                                                         *[t.data_ptr()] * 5, C.byref(ng), C.byref(npairs))
    assert rc == 1 and b"npeaks" in ctx.lib.chicdiff_hip_last_error(ctx.h)
    # no peaks / no survivor: status 0, zero groups
    empty = dict(base, peak_baitID=base["peak_baitID"][:0], peak_oeID=base["peak_oeID"][:0], scores=base["scores"][:, :0])
    for res in (run_device(ctx, empty, base["p"], False, 0.05, 1.0), run_device(ctx, base, base["p"], False, -1.0, 1.0)):
        assert res["ngroups"] == 0 and res["npairs"] == 0 and res["group_ptr"].cpu().tolist() == [0] and res["pair_row"].numel() == 0


@pytest.mark.gpu
def test_order_independence(ctx):
    g, case = _golden_table(), _golden_case()
    p = np.asarray(g["weighted_padj"])
    keys = np.stack([case["baitID"], case["minOE"], case["maxOE"]], axis=1)
    assert len(np.unique(keys, axis=0)) == len(keys)                                    # no ties: the pair order is fully determined
    a = run_device(ctx, case, p, False, 0.05, 1.0)
    b = run_device(ctx, case, p, False, 0.05, 1.0)
    perm = np.random.default_rng(3).permutation(len(p))
    c = run_device(ctx, dict(case, baitID=case["baitID"][perm], minOE=case["minOE"][perm], maxOE=case["maxOE"][perm]), p[perm], False, 0.05, 1.0)
    for k in ("group_peak", "group_ptr", "pair_row"):                                    # two identical calls: bit for bit
        assert np.array_equal(a[k].cpu().numpy(), b[k].cpu().numpy()), k
    for k in ("group_min_p", "group_delta"):
        assert same_bits(a[k].cpu().numpy(), b[k].cpu().numpy()), k
    for k in ("group_peak", "group_ptr"):
        assert np.array_equal(a[k].cpu().numpy(), c[k].cpu().numpy())
    assert same_bits(a["group_min_p"].cpu().numpy(), c["group_min_p"].cpu().numpy())
    assert same_bits(a["group_delta"].cpu().numpy(), c["group_delta"].cpu().numpy())
    assert np.array_equal(perm[c["pair_row"].cpu().numpy()], a["pair_row"].cpu().numpy()) and a["npairs"] > 0


@pytest.mark.gpu
@pytest.mark.parametrize("merged", [False, True])
def test_mirror(ctx, tmp_path, merged):
    import pandas as pd
    from chicdiff_amd import pipeline
    g = _golden_table()
    cols = ["baitID", "minOE", "maxOE", "regionID", "log2FoldChange", "weighted_padj", "OEstart", "OEend", "baitstart", "baitend"]
    output = pd.DataFrame({k: np.asarray(g[k]) for k in cols})
    case = _golden_case()
    P = 4000
    names = ["A", "B"] if merged else ["a1", "a2", "b1", "b2"]
    peaks = pd.DataFrame({"baitChr": 19, "baitStart": 1, "baitEnd": 2, "baitID": case["peak_baitID"][:P], "baitName": [f"gene{i}" for i in range(P)],
                          "oeChr": 19, "oeStart": 3, "oeEnd": 4, "oeID": case["peak_oeID"][:P], "oeName": ".", "dist": 1000})
    for j, c in enumerate(names):
        peaks[c] = np.round(case["scores"][j, :P], 4)   # four decimals: every text reader gives the same double
    path = str(tmp_path / "peaks.txt")
    peaks.to_csv(path, sep="\t", index=False, na_rep="NA")
    chicago = {"A": "a.Rds", "B": "b.Rds"} if merged else {"A": {"a1": "a1.Rds", "a2": "a2.Rds"}, "B": {"b1": "b1.Rds", "b2": "b2.Rds"}}
    settings = dict(chicagoData=chicago, targetColumns=names, score=SCORE, peakfiles=[path])
    mind = 10.0 if merged else 1.0   # merged: |col2 - col1| of the raw scores, no asinh
    got = pipeline.getCandidateInteractions(output, path, settings, minDeltaAsinhScore=mind, ctx=ctx)
    want = tw.candidates_table_literal({k: output[k].tolist() for k in cols}, {k: peaks[k].tolist() for k in peaks.columns},
                                       names[:len(names) // 2], names[len(names) // 2:], merged, SCORE, "weighted_padj", 0.05, mind)
    assert len(want) > 5 and len(got) == len(want)
    assert list(got.columns) == list(want[0]) == (["baitID", "oeID", "baitChr", "baitstart", "baitend", "baitName"] + names + [
        "min_weighted_padj", "deltaAsinhScore", "regionIDs", "log2FoldChanges", "weighted_padj", "OEranges"])
    for c in got.columns:
        w = [r[c] for r in want]
        if c == "deltaAsinhScore":
            if merged:
                assert same_bits(got[c].to_numpy(), w)
            else:
                import math
                scale = np.array([max(abs(math.asinh(math.fsum(r[n] for n in names[:2]) / 2)), abs(math.asinh(math.fsum(r[n] for n in names[2:]) / 2)))
                                  for r in want])
                assert (np.abs(got[c].to_numpy() - np.array(w)) <= DELTA_BOUND_UNITS * 2.0 ** -52 * scale).all()
        elif c in names or c == "min_weighted_padj":
            assert same_bits(got[c].to_numpy(), w), c
        else:
            assert got[c].tolist() == w, c
    if merged:   # no asinh: delta is the plain difference of the two columns
        assert np.array_equal(got["deltaAsinhScore"].to_numpy(), np.abs(got["B"].to_numpy() - got["A"].to_numpy()))
