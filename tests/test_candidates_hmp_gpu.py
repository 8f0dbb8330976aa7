"""getCandidateInteractions(method = "hmp") on the device (chicdiff_hip_candidate_interactions_method_dev, the binding and the mirror)
against the literal restatement tests/hmp_twin.candidates_hmp_literal.  Groups, pairs and counts are compared by equality, delta
in test_candidate_interactions' DELTA_BOUND_UNITS, the combined p in hmp_twin.LANDAU_BOUND_UNITS at the group's own z (the bound
of test_landau_tail_gpu.py) and bit for bit where the twin gives exactly 0 or 1."""
import ctypes as C
import functools
import math
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import candidates_inputs as ci  # noqa: E402
import hmp_twin as ht  # noqa: E402
from test_candidate_interactions import DELTA_BOUND_UNITS, _golden_case, _golden_table, _stack_case, run_device, same_bits  # noqa: E402

SCORE = ci.SCORE
CUTS = ((2.0, 0.0), (0.05, 1.0))      # every group survives the p filter / the reference's defaults
PEAKS, REGIONS = (1, 63, 64, 65, 513), (1, 2, 65, 700)


def mixed_p(n, seed):
    """Log-uniform values in (0, 1] with NaN, 1.5, exactly 1, 0, the smallest subnormal and 1e-300 mixed in."""
    rng = np.random.default_rng(seed)
    p = np.exp(rng.uniform(math.log(1e-6), 0.0, n))
    kind = rng.random(n)
    for lo, hi, v in ((0.0, 0.08, np.nan), (0.08, 0.12, 1.5), (0.12, 0.16, 1.0), (0.16, 0.18, 0.0), (0.18, 0.20, 5e-324), (0.20, 0.22, 1e-300)):
        p[(kind >= lo) & (kind < hi)] = v
    return p


@functools.lru_cache(maxsize=None)
def case_of(npeaks, nregions, big=False):
    if npeaks <= 0:   # 65 identical regions: L = 65 for both peaks
        case = _stack_case()
    else:
        case = ci.adversarial_case(npeaks, nregions, 99 if big else 1000 * npeaks + nregions, big_bait=big)
    if npeaks == -1:   # 300 identical regions whose p' are all 1: x = 1, z = (1 - log 300 - c) / (pi / 2) < -3.5, hm_p exactly 1
        case = {k: (np.resize(v, 300) if k in ("baitID", "minOE", "maxOE", "p") else v) for k, v in _stack_case().items()}
        return case, np.resize(np.array([np.nan, 1.5, 1.0]), 300)
    p = mixed_p(len(case["baitID"]), 7 + 31 * npeaks + nregions)
    return case, p


@functools.lru_cache(maxsize=None)
def twin_of(npeaks, nregions, big, pvcut, mind):
    case, p = case_of(npeaks, nregions, big)
    t = ht.candidates_hmp_literal(*ci.twin_args(case, p), SCORE, pvcut, mind)
    hm = np.array([g[1] for g in t["groups_all"]])
    # the condition of the keep-set comparison: no group's value within 1e-9 pvcut of the cut (the seeds are chosen so; no GPU needed)
    assert not (np.abs(hm - pvcut) <= 1e-9 * pvcut).any(), (npeaks, nregions, big, pvcut)
    return t


ALL_CASES = [(a, b, False) for a in PEAKS for b in REGIONS] + [(513, 700, True), (0, 65, False), (-1, 300, False)]


def test_no_twin_value_hangs_on_the_cut():
    """CPU: the precondition of every comparison below, and that the cases reach what they are for."""
    seen = set()
    for a, b, big in ALL_CASES:
        for pvcut, mind in CUTS:
            t = twin_of(a, b, big, pvcut, mind)
            seen |= {("zero", any(g[1] == 0.0 for g in t["groups_all"])), ("one", any(g[1] == 1.0 for g in t["groups_all"])),
                     ("mid", any(0.05 < g[1] < 1.0 for g in t["groups_all"])), ("kept", len(t["groups"]) > 0)}
    assert {("zero", True), ("one", True), ("mid", True), ("kept", True)} <= seen
    t = twin_of(513, 700, True, 2.0, 0.0)
    assert max(len(g[3]) for g in t["groups"]) > 64
    t = twin_of(0, 65, False, 2.0, 0.0)
    assert [len(g[3]) for g in t["groups"]] == [65, 65]
    assert [g[1] for g in twin_of(-1, 300, False, 2.0, 0.0)["groups"]] == [1.0, 1.0]
    # the 0.05 cut drops groups that the 2.0 cut keeps: the filter reads hm_p
    assert any(len(twin_of(a, b, big, 0.05, 1.0)["groups"]) < len(twin_of(a, b, big, 2.0, 0.0)["groups"]) for a, b, big in ALL_CASES)


@pytest.fixture(scope="module")
def ctx():
    import __graft_entry__ as g
    g.build()
    from chicdiff_amd import hip
    c = hip.HipContext(0)
    yield c
    c.close()


def compare_p(got, want, z, label):
    got, want, z = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64), np.asarray(z, dtype=np.float64)
    exact = (want == 0.0) | (want == 1.0)
    assert np.array_equal(got[exact], want[exact]), label
    if (~exact).any():
        units = np.abs(got[~exact] - want[~exact]) / ht.unit_at(z[~exact])
        print(f"{label}: combined p off by at most {units.max():.3f} units over {int((~exact).sum())} groups")
        assert units.max() <= ht.LANDAU_BOUND_UNITS, (label, float(units.max()))


def compare(res, twin, label):
    groups = twin["groups"]
    assert res["ngroups"] == len(groups) and res["npairs"] == sum(len(g[3]) for g in groups), (label, res["ngroups"], len(groups))
    assert np.array_equal(res["group_peak"].cpu().numpy(), np.array([g[0] for g in groups], dtype=np.int32)), label
    assert np.array_equal(res["group_ptr"].cpu().numpy(), np.concatenate([[0], np.cumsum([len(g[3]) for g in groups])]).astype(np.int64)), label
    assert np.array_equal(res["pair_row"].cpu().numpy(), np.array([r for g in groups for r in g[3]], dtype=np.int32)), label
    if groups:
        want = np.array([g[2] for g in groups])
        unit = 2.0 ** -52 * np.array([twin["scale"][g[0]] for g in groups])
        dev = np.abs(res["group_delta"].cpu().numpy() - want) / np.where(unit > 0, unit, 1.0)
        assert dev.max() <= DELTA_BOUND_UNITS, (label, float(dev.max()))
        compare_p(res["group_min_p"].cpu().numpy(), [g[1] for g in groups], twin["z_kept"], label)


@pytest.mark.gpu
@pytest.mark.parametrize("nregions", REGIONS)
@pytest.mark.parametrize("npeaks", PEAKS)
def test_adversarial(ctx, npeaks, nregions):
    case, p = case_of(npeaks, nregions)
    for pvcut, mind in CUTS:
        compare(run_device(ctx, case, p, False, pvcut, mind, method="hmp"), twin_of(npeaks, nregions, False, pvcut, mind),
                f"hmp/{npeaks}x{nregions}/{pvcut}/{mind}")


@pytest.mark.gpu
def test_more_than_64_matches_window_not_staged(ctx):
    case, p = case_of(513, 700, True)
    for pvcut, mind in CUTS:
        compare(run_device(ctx, case, p, False, pvcut, mind, method="hmp"), twin_of(513, 700, True, pvcut, mind), f"hmp/big/{pvcut}/{mind}")


@pytest.mark.gpu
def test_65_identical_regions(ctx):
    case, p = case_of(0, 65)
    for pvcut, mind in CUTS:
        compare(run_device(ctx, case, p, False, pvcut, mind, method="hmp"), twin_of(0, 65, False, pvcut, mind), f"hmp/stack/{pvcut}/{mind}")


@pytest.mark.gpu
def test_300_regions_of_p_one_give_exactly_one(ctx):
    case, p = case_of(-1, 300)
    for pvcut, mind in CUTS:
        compare(run_device(ctx, case, p, False, pvcut, mind, method="hmp"), twin_of(-1, 300, False, pvcut, mind), f"hmp/ones/{pvcut}/{mind}")


@pytest.mark.gpu
def test_order_independence(ctx):
    g, case = _golden_table(), _golden_case()
    p = np.asarray(g["padj"])
    keys = np.stack([case["baitID"], case["minOE"], case["maxOE"]], axis=1)
    assert len(np.unique(keys, axis=0)) == len(keys)                                    # no ties: the pair order is fully determined
    a = run_device(ctx, case, p, False, 0.05, 1.0, method="hmp")
    perm = np.random.default_rng(3).permutation(len(p))
    c = run_device(ctx, dict(case, baitID=case["baitID"][perm], minOE=case["minOE"][perm], maxOE=case["maxOE"][perm]), p[perm], False, 0.05, 1.0,
                   method="hmp")
    for k in ("group_peak", "group_ptr"):
        assert np.array_equal(a[k].cpu().numpy(), c[k].cpu().numpy())
    assert same_bits(a["group_min_p"].cpu().numpy(), c["group_min_p"].cpu().numpy())
    assert same_bits(a["group_delta"].cpu().numpy(), c["group_delta"].cpu().numpy())
    assert np.array_equal(perm[c["pair_row"].cpu().numpy()], a["pair_row"].cpu().numpy()) and a["npairs"] > 0


@pytest.mark.gpu
def test_unknown_method_is_refused(ctx):
    from chicdiff_amd import hip
    case, p = case_of(65, 65)
    with pytest.raises(ValueError, match=r"unknown method 'fisher' \(should be 'min' or 'hmp'\)"):
        run_device(ctx, case, p, False, 0.05, 1.0, method="fisher")
    for m in (2, -1):
        with pytest.raises(hip.ChicdiffHipError, match=rf"method = {m} \(CHICDIFF_CAND_MIN = 0 or CHICDIFF_CAND_HMP = 1\)"):
            run_device(ctx, case, p, False, 0.05, 1.0, method=m)


@pytest.mark.gpu
def test_min_through_the_new_entry_point_equals_the_old_one(ctx):
    torch = ctx.torch
    case = ci.adversarial_case(513, 700, 513700)
    new = run_device(ctx, case, case["p"], False, 1.0, 0.0, method="min")                # the binding calls ..._method_dev with 0
    dev = lambda a, dt: torch.from_numpy(np.ascontiguousarray(a, dtype=dt)).to(ctx.device)
    P, n = len(case["peak_baitID"]), len(case["baitID"])
    args = [dev(case[k], np.int32) for k in ("baitID", "minOE", "maxOE")] + [dev(case["p"], np.float64)]
    peaks = [dev(case["peak_baitID"], np.int32), dev(case["peak_oeID"], np.int32), dev(case["scores"], np.float64)]
    gpeak, gptr = torch.empty(P, dtype=torch.int32, device=ctx.device), torch.empty(P + 1, dtype=torch.int64, device=ctx.device)
    gmin, gdelta = (torch.empty(P, dtype=torch.float64, device=ctx.device) for _ in range(2))
    pairs = torch.empty(16 * P, dtype=torch.int32, device=ctx.device)
    ng, npairs = C.c_int64(0), C.c_int64(0)
    rc = ctx.lib.chicdiff_hip_candidate_interactions_dev(ctx.h, *[t.data_ptr() for t in args], n, *[t.data_ptr() for t in peaks], P, 4, 2, 2, 0,
                                                         SCORE, 1.0, 0.0, pairs.numel(), gpeak.data_ptr(), gptr.data_ptr(), gmin.data_ptr(),
                                                         gdelta.data_ptr(), pairs.data_ptr(), C.byref(ng), C.byref(npairs))
    assert rc == 0 and (ng.value, npairs.value) == (new["ngroups"], new["npairs"]) and ng.value > 50
    g, m = ng.value, npairs.value
    assert torch.equal(gpeak[:g], new["group_peak"]) and torch.equal(gptr[:g + 1], new["group_ptr"]) and torch.equal(pairs[:m], new["pair_row"])
    assert same_bits(gmin[:g].cpu().numpy(), new["group_min_p"].cpu().numpy())
    assert same_bits(gdelta[:g].cpu().numpy(), new["group_delta"].cpu().numpy())
    assert not np.isnan(new["group_min_p"].cpu().numpy()).any()                          # "min": a group whose minimum is NA is dropped (:2161)
    hm = run_device(ctx, case, case["p"], False, 2.0, 0.0, method="hmp")
    assert not np.isnan(hm["group_min_p"].cpu().numpy()).any() and hm["ngroups"] > g   # "hmp" counts NA as 1: those groups are back


@pytest.mark.gpu
def test_mirror(ctx, tmp_path):
    import pandas as pd
    from chicdiff_amd import pipeline
    g = _golden_table()
    cols = ["baitID", "minOE", "maxOE", "regionID", "log2FoldChange", "padj", "OEstart", "OEend", "baitstart", "baitend"]
    output = pd.DataFrame({k: np.asarray(g[k]) for k in cols})
    assert np.isnan(output["padj"].to_numpy()).any()                                     # NA rows: :2136 replaces them
    case = _golden_case()
    P = 4000
    names = ["a1", "a2", "b1", "b2"]
    peaks = pd.DataFrame({"baitChr": 19, "baitStart": 1, "baitEnd": 2, "baitID": case["peak_baitID"][:P], "baitName": [f"gene{i}" for i in range(P)],
                          "oeChr": 19, "oeStart": 3, "oeEnd": 4, "oeID": case["peak_oeID"][:P], "oeName": ".", "dist": 1000})
    for j, c in enumerate(names):
        peaks[c] = np.round(case["scores"][j, :P], 4)
    path = str(tmp_path / "peaks.txt")
    peaks.to_csv(path, sep="\t", index=False, na_rep="NA")
    settings = dict(chicagoData={"A": {"a1": "a1.Rds", "a2": "a2.Rds"}, "B": {"b1": "b1.Rds", "b2": "b2.Rds"}}, targetColumns=names, score=SCORE,
                    peakfiles=[path])
    pvcut = 2.0   # every group survives the p filter, so the groups whose padj is NA are in the table
    got = pipeline.getCandidateInteractions(output, path, settings, pcol="padj", method="hmp", minDeltaAsinhScore=1.0, pvcut=pvcut, ctx=ctx)
    want, z = ht.candidates_table_hmp_literal({k: output[k].tolist() for k in cols}, {k: peaks[k].tolist() for k in peaks.columns},
                                              names[:2], names[2:], False, SCORE, "padj", pvcut, 1.0)
    assert len(want) > 5 and len(got) == len(want)
    assert list(got.columns) == list(want[0]) == (["baitID", "oeID", "baitChr", "baitstart", "baitend", "baitName"] + names + [
        "hm_padj", "deltaAsinhScore", "regionIDs", "log2FoldChanges", "padj", "OEranges"])
    for c in got.columns:
        w = [r[c] for r in want]
        if c == "deltaAsinhScore":
            scale = np.array([max(abs(math.asinh(math.fsum(r[n] for n in names[:2]) / 2)), abs(math.asinh(math.fsum(r[n] for n in names[2:]) / 2)))
                              for r in want])
            assert (np.abs(got[c].to_numpy() - np.array(w)) <= DELTA_BOUND_UNITS * 2.0 ** -52 * scale).all()
        elif c == "hm_padj":
            compare_p(got[c].to_numpy(), w, z, "mirror")
        elif c in names:
            assert same_bits(got[c].to_numpy(), w), c
        else:
            assert got[c].tolist() == w, c
    pasted = ",".join(got["padj"].tolist()).split(",")
    assert "NA" not in pasted and "1" in pasted                                          # the replaced values, not the table's NA
    # the defaults' cut: the same table, filtered on hm_padj
    cut = pipeline.getCandidateInteractions(output, path, settings, pcol="padj", method="hmp", minDeltaAsinhScore=1.0, ctx=ctx)
    keep = [r for r in want if r["hm_padj"] <= 0.05]
    assert not any(abs(r["hm_padj"] - 0.05) <= 0.05e-9 for r in want)
    assert 0 < len(keep) < len(want) and cut["regionIDs"].tolist() == [r["regionIDs"] for r in keep]
