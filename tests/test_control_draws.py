"""The seeded control draws, CPU side: the numpy twin (tests/control_twin.py) against known answers and against the distribution
of the unseeded host path, and the interface through every layer."""
import inspect
import os
import re

import numpy as np
import pytest

import control_inputs as ci
import control_twin as tw

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("counter, key, expected", [
    ((0, 0, 0, 0), (0, 0), "6627e8d5 e169c58d bc57ac4c 9b00dbd8"),
    ((0xffffffff,) * 4, (0xffffffff,) * 2, "408f276d 41c83b0e a20bc7c6 6d5451fd"),
    ((0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344), (0xa4093822, 0x299f31d0), "d16cfe09 94fdcceb 5001e420 24126ea1"),
])
def test_philox_known_answers(counter, key, expected):
    out = tw.philox4x32(*counter, *key)
    assert " ".join(f"{int(w[0]):08x}" for w in out) == expected


def test_draw_words_use_the_stated_counter_and_key_layout():
    k, seed = (5 << 32) | 9, (0x299f31d0 << 32) | 0xa4093822
    a = tw.draw_words(seed, [k], 3, 1)
    b = tw.philox4x32(9, 5, 3, 1, 0xa4093822, 0x299f31d0)
    assert all(int(x[0]) == int(y[0]) for x, y in zip(a, b))


def test_uniform_never_reaches_zero_or_one():
    assert tw.uniform(0, 0) == 2.0 ** -53
    assert tw.uniform(0xffffffff, 0xffffffff) == 1.0 - 2.0 ** -53
    r = np.random.default_rng(0).integers(0, 2 ** 32, (2, 1000), dtype=np.uint64)
    u = tw.uniform(r[0], r[1])
    assert (u > 0).all() and (u < 1).all()


def test_qnorm_against_ndtri():
    from scipy.special import ndtri
    rng = np.random.default_rng(5)
    r = rng.integers(0, 2 ** 32, (2, 100_000), dtype=np.uint64)
    r[:, 0], r[:, 1] = 0, 0xffffffff                                               # both ends of the uniform
    u = tw.uniform(r[0], r[1])
    u[2:2002] = np.exp(rng.uniform(np.log(2.0 ** -53), np.log(0.075), 2000))       # the tails, down to the smallest u
    u[2002:4002] = 1.0 - u[2:2002]
    u[4002:4006] = [0.075, 0.925, 0.5 - 2.0 ** -53, 0.5 + 2.0 ** -53]
    u = u[u != 0.5]
    z, ref = tw.qnorm(u), ndtri(u)
    err = np.abs(z - ref) / np.abs(ref)
    worst = int(np.argmax(err))
    assert err[worst] <= 2.0 ** -44, f"worst relative error {err[worst]:.3e} at u = {u[worst]!r} (bound 2^-44 = {2.0 ** -44:.3e})"
    assert tw.qnorm(0.5)[0] == 0.0 and (np.sign(z) == np.sign(u - 0.5)).all()


class _HostOnlyContext:
    """What pipeline.getControlRegionUniverse touches of a HipContext when only the drawn pairs matter: the expansion is not run,
    the pairs handed to it are kept."""

    def __init__(self):
        import torch
        self.torch, self.device = torch, torch.device("cpu")

    def region_universe(self, d_bait, d_oe, RUexpand, d_chr_of):
        t = self.torch
        self.pairs = (d_bait.numpy().copy(), d_oe.numpy().copy())
        e = lambda dt: t.empty(0, dtype=dt)
        return dict(region_ptr=t.zeros(d_bait.numel() + 1, dtype=t.int64), minOE=e(t.int32), maxOE=e(t.int32), baitID=e(t.int32),
                    regionID=e(t.int32), otherEndID=e(t.int32))


def test_twin_realises_the_distribution_of_the_host_path(tmp_path):
    """20 011 draws of the twin (seed 1) against 20 011 of the unseeded host path (rng = default_rng(11)) on the same universe: the
    offsets oeID - baitID per chromosome by a two-sample KS test, the bait frequencies by chi-square.  Both sides are seeded, so
    the p-values are fixed numbers."""
    import torch
    from scipy import stats
    from chicdiff_amd import pipeline
    d = ci.design()
    n = 20011
    ru_b, ru_r, ru_o = ci.ru_rows(n, d)
    assert len(np.unique(ru_r)) == n and ru_r.max() > n                             # the empty regions' IDs are missing
    contact = tw.max_contact(ru_b, ru_o, d["chr_of"], len(d["names"]))
    assert {str(nm): int(c) for nm, c in zip(d["names"], contact)} == ci.EXPECTED_CONTACT
    RU = dict(baitID=torch.from_numpy(ru_b), regionID=torch.from_numpy(ru_r), otherEndID=torch.from_numpy(ru_o))
    ctx = _HostOnlyContext()
    pipeline.getControlRegionUniverse(ci.settings(tmp_path, d), RU, ctx, rng=np.random.default_rng(11))
    hb, ho = (a.astype(np.int64) for a in ctx.pairs)
    t = tw.control_draws(1, n, d["bmap_id"], d["bmap_chr"], d["chr_min"], d["chr_max"], contact)
    tb, to = t["baitID"].astype(np.int64), t["oeID"].astype(np.int64)
    report = {}
    for c, name in enumerate(d["names"]):
        on = lambda b: (b >= d["chr_min"][c]) & (b <= d["chr_max"][c])
        if contact[c] == 0:
            assert not on(tb).any() and not on(hb).any()                            # baits of a chromosome without a contact are dropped
            continue
        p = stats.ks_2samp((to - tb)[on(tb)], (ho - hb)[on(hb)]).pvalue
        report[f"ks {name}"] = p
        assert p > 1e-3, report
    baits = d["bmap_id"][contact[d["bmap_chr"]] > 0]
    table = np.stack([np.bincount(np.searchsorted(baits, x), minlength=len(baits)) for x in (tb, hb)])
    p = stats.chi2_contingency(table).pvalue
    report["chi2 baits"] = p
    assert p > 1e-3, report
    assert abs(len(tb) - len(hb)) < 5 * np.sqrt(n * 0.04)                           # both drop the ~4 % of draws that land on chromosome "1"
    print(report)
    # what the layout exercises (the figures the GPU test's description quotes)
    assert t["attempts"].max() <= 12 and 0.10 < t["reflected"].sum() / n < 0.22 and 0.02 < 1 - t["m"] / n < 0.06
    assert (np.abs(to - tb) == 1).sum() > 500
    assert t["m"] - len(np.unique(tb * 4096 + to)) > 2000


@pytest.mark.parametrize("seed", ci.SEEDS)
def test_no_draw_of_the_gpu_cases_sits_on_a_rounding_boundary(seed):
    """The GPU test allows a draw to differ from the twin only where z * std lies within 2^-40 of a half-integer; for the shapes
    and seeds it runs, the twin has no such attempt, so there every draw must be equal."""
    d = ci.design()
    contact = np.array([ci.EXPECTED_CONTACT[str(nm)] for nm in d["names"]])
    t = tw.control_draws(seed, max(ci.SHAPES), d["bmap_id"], d["bmap_chr"], d["chr_min"], d["chr_max"], contact)   # draw k does not depend on n
    assert tw.rounding_band(t["x"]) == []
    assert ((t["draw_oe"] >= d["chr_min"][t["draw_chr"]]) & (t["draw_oe"] <= d["chr_max"][t["draw_chr"]]))[t["kept"]].all()
    assert (t["draw_oe"] != t["draw_bait"])[t["kept"]].all()


def test_interface_through_every_layer():
    """The C header declares the entry point, the binding exports and wraps it, and both pipeline functions take the seed."""
    from chicdiff_amd import hip, pipeline, post
    hdr = open(os.path.join(ROOT, "include", "chicdiff_hip.h")).read()
    assert re.search(r"\bint chicdiff_hip_control_draws_dev\s*\(", hdr)
    assert "CHICDIFF_CONTROL_MAX_CHR" in hdr and "CHICDIFF_CONTROL_MAX_ATTEMPTS 256" in hdr
    assert "chicdiff_hip_control_draws_dev" in hip.EXPORTS and callable(hip.HipContext.control_draws)
    p = inspect.signature(pipeline.getControlRegionUniverse).parameters
    assert list(p)[:3] == ["chicdiff_settings", "RU", "ctx"] and p["rng"].default is None and p["seed"].default is None
    assert inspect.signature(pipeline.chicdiffPipeline).parameters["control_seed"].default is None
    with pytest.raises(ValueError, match="rng.*seed|seed.*rng"):
        pipeline.getControlRegionUniverse({}, {}, None, rng=np.random.default_rng(0), seed=1)
    assert "control_kernels.hip" in open(os.path.join(ROOT, "chicdiff_amd", "csrc", "Makefile")).read()
    assert inspect.signature(post.getRegionUniverse).parameters                     # (device tensors are accepted: tested on the GPU)
