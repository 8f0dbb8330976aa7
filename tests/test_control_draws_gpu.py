"""The seeded control draws on the device (chicdiff_hip_control_draws_dev) against the numpy twin (tests/control_twin.py) on the
layout of tests/control_inputs.py: one lane, either side of a wave and of a workgroup, several workgroups; a seed that uses the
high key word.  Draw k depends on (seed, k) only, so the twin draws the largest shape once per seed and every shape reads a prefix."""
import collections
import ctypes as C
import functools
import json
import os

import numpy as np
import pytest

import control_inputs as ci
import control_twin as tw

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
D = ci.design()
CONTACT = np.array([ci.EXPECTED_CONTACT[str(nm)] for nm in D["names"]])


@pytest.fixture(scope="module")
def ctx():
    import __graft_entry__ as g
    g.build()
    from chicdiff_amd import hip
    c = hip.HipContext(0)
    yield c
    c.close()


@functools.lru_cache(maxsize=None)
def twin_draws(seed):
    return tw.control_draws(seed, max(ci.SHAPES), D["bmap_id"], D["bmap_chr"], D["chr_min"], D["chr_max"], CONTACT)


def twin_pairs(seed, n, contact=CONTACT):
    """The twin's sorted kept pairs of the first n draws (chromosomes without a contact in ``contact`` dropped)."""
    t = twin_draws(seed)
    kept = t["kept"][:n] & (np.asarray(contact)[np.maximum(t["draw_chr"][:n], 0)] > 0)
    b, o = t["draw_bait"][:n][kept], t["draw_oe"][:n][kept]
    order = np.lexsort((o, b))
    return b[order].astype(np.int32), o[order].astype(np.int32), kept


_UNIVERSES = {}


def universe(ctx, n):
    """RU of ci.peaks(n) from the device expansion, and its rows on the host (for the twin's row-level maxima)."""
    if n not in _UNIVERSES:
        from chicdiff_amd import pipeline, post
        pb, po = ci.peaks(n)
        ru = pipeline.RegionUniverse(post.getRegionUniverse(ctx, pb, po, ci.RUEXPAND, D["chrom"], D["ids"]))
        rows = tuple(ru[k].cpu().numpy() for k in ("csr_baitID", "csr_regionID", "csr_otherEndID"))
        _UNIVERSES[n] = (ru, rows)
    return _UNIVERSES[n]


def draws(ctx, ru, seed, d=D):
    torch = ctx.torch
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a, dtype=np.int32)).to(ctx.device)
    return ctx.control_draws(ru["csr_baitID"], ru["region_ptr"], ru["minOE"], ru["maxOE"], dev(d["bmap_id"]), dev(d["bmap_chr"]),
                             d["chr_min"], d["chr_max"], seed)


@pytest.mark.parametrize("seed", ci.SEEDS)
@pytest.mark.parametrize("n", ci.SHAPES)
def test_draws_equal_the_twin(ctx, n, seed):
    ru, (rb, rr, ro) = universe(ctx, n)
    r = draws(ctx, ru, seed)
    # 1. the region-level maxima and count against the ROW-level definition (chicdiff.R:463-466)
    contact = tw.max_contact(rb, ro, D["chr_of"], len(D["names"]))
    assert np.array_equal(r["max_contact"].cpu().numpy(), contact), (r["max_contact"].cpu().numpy(), contact)
    assert r["n_regions"] == len(np.unique(rr)) == n and ru["region_ptr"].numel() - 1 >= n + len(ci.EMPTY_PEAKS)
    if n >= 3:
        assert {str(nm): int(c) for nm, c in zip(D["names"], contact)} == ci.EXPECTED_CONTACT
    # 2. every kept pair, in order
    eb, eo, kept = twin_pairs(seed, n, contact)
    gb, go = r["baitID"].cpu().numpy(), r["oeID"].cpu().numpy()
    assert r["m"] == len(eb) == int(kept.sum()) and len(gb) == r["m"]          # a draw is dropped by its bait alone: m never differs
    band = [j for j in tw.rounding_band(twin_draws(seed)["x"][:n]) if kept[j]]
    assert len(band) <= 1, band
    if not (np.array_equal(gb, eb) and np.array_equal(go, eo)):
        # refereed: a draw may differ only where the twin's z * std sits within 2^-40 of a half-integer (a last-bit difference of the
        # logarithm could turn the rounding there), at most one per test; every other pair must be there
        t = twin_draws(seed)
        want = collections.Counter(zip(eb.tolist(), eo.tolist()))
        got = collections.Counter(zip(gb.tolist(), go.tolist()))
        missing = want - got
        allowed = collections.Counter((int(t["draw_bait"][j]), int(t["draw_oe"][j])) for j in band)
        assert not (missing - allowed), f"pairs of the twin that the device lacks outside the refereed list: {dict(missing - allowed)}"
        assert sum((got - want).values()) <= len(band) and {b for b, _ in (got - want)} <= {b for b, _ in allowed}
        assert (np.diff(gb.astype(np.int64) * 4096 + go) >= 0).all()
    # 4. (first half) every seed of a region lies on its bait's chromosome and is not the bait
    code = D["chr_of"][gb]
    assert (go >= D["chr_min"][code]).all() and (go <= D["chr_max"][code]).all() and (go != gb).all()
    assert (D["chr_of"][go] == code).all() and (contact[code] > 0).all()


def test_device_qnorm_against_the_twin(ctx):
    """selftest op 9 = AS 241 as the draw kernel calls it: the middle takes only + x / and must give numpy's bits; the tails take
    sqrt and the polynomial logarithm (0.74 ulp) and are held to 2^-44 relative."""
    torch = ctx.torch
    rng = np.random.default_rng(17)
    r = rng.integers(0, 2 ** 32, (2, 200_000), dtype=np.uint64)
    r[:, 0], r[:, 1] = 0, 0xffffffff
    u = tw.uniform(r[0], r[1])
    u[2:20002] = np.exp(rng.uniform(np.log(2.0 ** -53), np.log(0.075), 20000))
    u[20002:40002] = 1.0 - u[2:20002]
    u[40002:40008] = [0.075, 0.925, np.nextafter(0.075, 0), np.nextafter(0.925, 1), 0.5, 0.5 - 2.0 ** -53]
    want = tw.qnorm(u)
    got = ctx.selftest_math(9, torch.from_numpy(u).to(ctx.device)).cpu().numpy()
    mid = np.abs(u - 0.5) <= 0.425
    assert mid.sum() > 100_000 and (~mid).sum() > 40_000
    nbits = int((got[mid].view(np.int64) != want[mid].view(np.int64)).sum())
    err = np.abs(got[~mid] - want[~mid]) / np.abs(want[~mid])
    worst = int(np.argmax(err))
    rec = dict(points=int(len(u)), middle_points=int(mid.sum()), middle_bit_mismatches=nbits, tail_points=int((~mid).sum()),
               tail_worst_relative_error=float(err[worst]), tail_worst_at_u=float(u[~mid][worst]), tail_bit_mismatches=int((got[~mid] != want[~mid]).sum()),
               bound=2.0 ** -44)
    print(rec)
    out = os.environ.get("CHICDIFF_ACCURACY_OUT")   # a directory: keep the figures behind the two assertions (-> profiles/r17_control_draws_accuracy.json)
    if out:
        os.makedirs(out, exist_ok=True)
        with open(os.path.join(out, "r17_control_draws_accuracy.json"), "w") as f:
            json.dump(rec, f, indent=1)
    assert nbits == 0, rec
    assert err[worst] <= 2.0 ** -44, rec


@pytest.mark.parametrize("n, seed", [(257, ci.SEEDS[0]), (4097, ci.SEEDS[1])])
def test_control_universe_through_the_pipeline(ctx, tmp_path, n, seed):
    """getControlRegionUniverse(seed=...): the expanded control universe equals the twin's pairs pushed through the same expansion,
    bit for bit; its regions are 1 .. m; the CSV of saveAuxData holds the same rows."""
    import pandas as pd
    from chicdiff_amd import pipeline, post
    ru, _ = universe(ctx, n)
    s = ci.settings(tmp_path)
    s["saveAuxData"] = [True]
    got = pipeline.getControlRegionUniverse(s, ru, ctx, seed=seed)
    eb, eo, _ = twin_pairs(seed, n)
    want = post.getRegionUniverse(ctx, eb, eo, ci.RUEXPAND, D["chrom"], D["ids"])
    for k, v in want.items():
        assert ctx.torch.equal(got[k], v), k
    m = len(eb)
    assert np.array_equal(got["peak_baitID"], eb) and got["region_ptr"].numel() == m + 1
    rid = got["csr_regionID"].cpu().numpy()
    assert rid.min() >= 1 and rid.max() <= m and (np.diff(rid) >= 0).all() and len(np.unique(rid)) > 0.9 * m
    csv = pd.read_csv(s["outprefix"][0] + "_ControlRegionUniverse.csv")
    assert list(csv.columns) == ["baitID", "regionID", "otherEndID"] and np.array_equal(csv["otherEndID"].to_numpy(), got["otherEndID"].cpu().numpy())


def test_same_seed_same_tensors_other_seed_other_tensors(ctx):
    ru, _ = universe(ctx, 4097)
    a, b, c = draws(ctx, ru, 99), draws(ctx, ru, 99), draws(ctx, ru, 100)
    assert a["m"] == b["m"] and ctx.torch.equal(a["baitID"], b["baitID"]) and ctx.torch.equal(a["oeID"], b["oeID"])
    assert ctx.torch.equal(a["max_contact"], c["max_contact"]) and a["n_regions"] == c["n_regions"] == 4097
    assert a["m"] != c["m"] or not (ctx.torch.equal(a["baitID"], c["baitID"]) and ctx.torch.equal(a["oeID"], c["oeID"]))


def test_refusals(ctx, tmp_path):
    from chicdiff_amd import hip, pipeline
    torch = ctx.torch
    ru, _ = universe(ctx, 65)
    dev = lambda a, dt=np.int32: torch.from_numpy(np.ascontiguousarray(a, dtype=dt)).to(ctx.device)
    args = lambda **kw: {**dict(d_ru_baitID=ru["csr_baitID"], d_region_ptr=ru["region_ptr"], d_minOE=ru["minOE"], d_maxOE=ru["maxOE"],
                                d_bmap_id=dev(D["bmap_id"]), d_bmap_chr=dev(D["bmap_chr"]), chr_min=D["chr_min"], chr_max=D["chr_max"], seed=1), **kw}
    # an empty baitmap: the binding refuses it, and so does the library when called directly
    with pytest.raises(ValueError, match="nb = 0"):
        ctx.control_draws(**args(d_bmap_id=dev([]), d_bmap_chr=dev([])))
    n = ru["region_ptr"].numel() - 1
    out = torch.empty(n, dtype=torch.int32, device=ctx.device)
    lo, hi = (np.ascontiguousarray(a, dtype=np.int32) for a in (D["chr_min"], D["chr_max"]))
    P, cnt = C.POINTER(C.c_int32), (C.c_int64(0), C.c_int64(0))
    rc = ctx.lib.chicdiff_hip_control_draws_dev(ctx.h, ru["csr_baitID"].data_ptr(), ru["csr_baitID"].numel(), ru["region_ptr"].data_ptr(),
                                                ru["minOE"].data_ptr(), ru["maxOE"].data_ptr(), n, out.data_ptr(), out.data_ptr(), 0,
                                                lo.ctypes.data_as(P), hi.ctypes.data_as(P), 4, 1, out.data_ptr(), out.data_ptr(), out.data_ptr(),
                                                C.byref(cnt[0]), C.byref(cnt[1]))
    assert rc != 0 and "nb = 0" in ctx.lib.chicdiff_hip_last_error(ctx.h).decode()
    for bad in (True, 1.5, -1, 2 ** 64):
        with pytest.raises(ValueError, match="seed"):
            ctx.control_draws(**args(seed=bad))
    with pytest.raises(ValueError, match="d_minOE"):
        ctx.control_draws(**args(d_minOE=ru["minOE"][:-1]))
    with pytest.raises(ValueError, match="d_bmap_chr"):
        ctx.control_draws(**args(d_bmap_chr=dev(D["bmap_chr"], np.int64)))
    # a baitmap code beyond the chromosome tables; overlapping chromosome ranges; more chromosomes than the LDS tables hold
    code = D["bmap_chr"].copy()
    code[5] = 4
    with pytest.raises(hip.ChicdiffHipError, match="row 5 of the baitmap"):
        ctx.control_draws(**args(d_bmap_chr=dev(code)))
    with pytest.raises(hip.ChicdiffHipError, match="overlap"):
        ctx.control_draws(**args(chr_max=np.array([1100, 450, 1000, 1060])))
    hdr = open(os.path.join(ROOT, "include", "chicdiff_hip.h")).read()
    cap = int(hdr.split("#define CHICDIFF_CONTROL_MAX_CHR")[1].split()[0])
    with pytest.raises(hip.ChicdiffHipError, match=f"nchr <= {cap}"):
        ctx.control_draws(**args(chr_min=np.arange(cap + 1) * 2 + 1, chr_max=np.arange(cap + 1) * 2 + 2))
    # no non-empty region
    with pytest.raises(hip.ChicdiffHipError, match="no non-empty region"):
        ctx.control_draws(**args(d_region_ptr=ru["region_ptr"] * 0))
    # offsets that leave the rows
    with pytest.raises(hip.ChicdiffHipError, match="region_ptr"):
        ctx.control_draws(**args(d_region_ptr=ru["region_ptr"] + 5))
    # a bait whose chromosome is itself: min = max = bait leaves no valid distance — every one of the 256 attempts of each draw is
    # rejected (a bounded loop), and the call names the first draw
    with pytest.raises(hip.ChicdiffHipError, match=r"draw k = 0 \(bait 51 on chromosome code 1, IDs 51 \.\. 51\).*256 attempts"):
        ctx.control_draws(dev([51, 51, 51]), dev([0, 1, 2, 3], np.int64), dev([53, 53, 53]), dev([53, 53, 53]), dev([51]), dev([1]),
                          np.array([1, 51]), np.array([50, 51]), 3)
    # no chromosome with a contact: nothing is kept, and that is not an error
    r = ctx.control_draws(dev([60]), dev([0, 1], np.int64), dev([62]), dev([62]), dev([51]), dev([1]), np.array([1, 51]), np.array([50, 51]), 3)
    assert r["m"] == 0 and r["n_regions"] == 1 and r["baitID"].numel() == 0 and r["max_contact"].cpu().tolist() == [0, 0]
    # both generators given
    with pytest.raises(ValueError, match="not both"):
        pipeline.getControlRegionUniverse(ci.settings(tmp_path), ru, ctx, rng=np.random.default_rng(1), seed=1)


def test_pipeline_with_a_control_seed_is_repeatable(ctx, tmp_path, monkeypatch):
    """chicdiffPipeline(control_seed=7) twice: identical result tables, the draws taken on the device; without a seed the host
    path runs as before."""
    import pandas as pd
    from chicdiff_amd import pipeline
    from pipeline_inputs import make_experiment, quantile_ihw, read_chicago_pickle
    settings, _ = make_experiment(tmp_path, npeaks=1200, with_chinput=True)
    calls = []
    real = ctx.control_draws
    monkeypatch.setattr(ctx, "control_draws", lambda *a, **k: calls.append(a[-1]) or real(*a, **k))
    run = lambda **kw: pipeline.chicdiffPipeline(settings, ctx=ctx, read_chicago=read_chicago_pickle, ihw=quantile_ihw(),
                                                 rng=np.random.default_rng(11), **kw)
    a, b = run(control_seed=7), run(control_seed=7)
    assert calls == [7, 7]
    pd.testing.assert_frame_equal(a, b, check_exact=True)
    assert len(a) > 100 and a["weighted_padj"].notna().any()
    c = run()
    assert calls == [7, 7] and list(c.columns) == list(a.columns) and len(c) == len(a)
