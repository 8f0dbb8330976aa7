"""Training the IHW weights on the device (chicdiff_hip_ihw_train_dev, chicdiff_hip_selftest_ihw_knots_dev) against the twin
(tests/ihw_twin.py), bit for bit: every group, fold, knot (x as bits, count) and weight (as bits), at every chunk length the library
accepts, on the cases of tests/ihw_inputs.py.  Every operation of the rule is an integer operation, a double operation in a stated
order or an exact comparison, so no tolerance stands between the two."""
import numpy as np
import pytest

import ihw_inputs as ii
import ihw_twin as tw

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx():
    import __graft_entry__ as g
    g.build()
    from chicdiff_amd import hip
    c = hip.HipContext(0)
    yield c
    c.close()


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def dev(ctx, a):
    return ctx.torch.from_numpy(np.ascontiguousarray(a, dtype=np.float64)).to(ctx.device)


def assert_equals_twin(ctx, name, L):
    k, t = ii.cases()[name], ii.twin(name)
    dp, dc = dev(ctx, k["p"]), dev(ctx, k["cov"])
    r = ctx.ihw_train(dp, dc, alpha=k["alpha"], nbins=k["nbins"] or None, nfolds=k["nfolds"], seed=k["seed"], chunk_len=L)
    assert (r["m"], r["nbins"], r["chunk_len"]) == (t["m"], t["nbins"], L)
    assert np.array_equal(r["group"].cpu().numpy().astype(np.int64), t["group"]), name
    assert np.array_equal(r["fold"].cpu().numpy().astype(np.int64), t["fold"]), name
    kn = ctx.selftest_ihw_knots(dp, dc, nbins=k["nbins"] or None, nfolds=k["nfolds"], seed=k["seed"], chunk_len=L)
    assert kn["nbins"] == t["nbins"] and kn["ptr"][0] == 0 and kn["ptr"][-1] == len(kn["x"])
    for f in range(k["nfolds"]):
        for g in range(t["nbins"]):
            q = f * t["nbins"] + g
            lo, hi = kn["ptr"][q], kn["ptr"][q + 1]
            want = t["knots"][(f, g)]
            assert np.array_equal(bits(kn["x"][lo:hi]), bits([x for x, _ in want])), (name, L, f, g)
            assert np.array_equal(kn["c"][lo:hi], np.array([c for _, c in want], dtype=np.int32)), (name, L, f, g)
    assert np.array_equal(r["nseg"], t["nseg"])
    assert np.array_equal(r["H"], t["H"].astype(np.float64))
    assert np.array_equal(bits(r["T"]), bits(t["T"])), (name, L, r["T"], t["T"])
    assert r["weights"].shape == t["weights"].shape
    assert np.array_equal(bits(r["weights"]), bits(t["weights"])), (name, L, r["weights"], t["weights"])
    return r


@pytest.mark.parametrize("L", ii.CHUNKS)
@pytest.mark.parametrize("name", sorted(ii.cases()))
def test_device_equals_twin(ctx, name, L):
    assert_equals_twin(ctx, name, L)


def test_caps_and_default_chunk(ctx):
    from chicdiff_amd import hip
    caps = hip.ihw_caps()
    assert tuple(caps["chunk_lens"]) == ii.CHUNKS and len(caps["chunk_lens"]) >= 3 and min(caps["chunk_lens"]) <= 8
    k = ii.cases()["n1025"]
    r = ctx.ihw_train(dev(ctx, k["p"]), dev(ctx, k["cov"]), alpha=k["alpha"], nbins=k["nbins"], nfolds=k["nfolds"], seed=k["seed"])
    assert r["chunk_len"] == caps["chunk_lens"][-1]
    assert np.array_equal(bits(r["weights"]), bits(ii.twin("n1025")["weights"]))


def test_repeated_calls_on_one_context(ctx):
    """Small after large after small, and a refusal in between: the grow-only scratch keeps nothing of the call before."""
    first = assert_equals_twin(ctx, "n257_one_bin", 4)
    assert_equals_twin(ctx, "n20011", 32)
    with pytest.raises(Exception, match="outside"):
        ctx.ihw_train(dev(ctx, [0.5, 1.5]), dev(ctx, [1.0, 2.0]), nbins=1, nfolds=2, seed=1)
    again = assert_equals_twin(ctx, "n257_one_bin", 4)
    assert np.array_equal(bits(first["weights"]), bits(again["weights"]))
    assert_equals_twin(ctx, "m8_folds16", 128)


def test_planted_properties_hold_on_the_device(ctx):
    r = assert_equals_twin(ctx, "m8_folds16", 4)
    assert (r["H"] == 0).any()                                       # an empty hold-out fold: every weight of it is 1
    assert np.all(r["weights"][:, r["H"] == 0] == 1.0)
    r = assert_equals_twin(ctx, "null_T0", 4)
    assert np.all(r["T"] == 0.0) and np.all(r["weights"] == 1.0)
    r = assert_equals_twin(ctx, "sweep_whole_segment", 4)
    assert np.array_equal(r["T"], r["H"] * 0.25)
    r = assert_equals_twin(ctx, "grid_collinear", 4)
    assert np.all(r["nseg"] == 1)                                    # every inner point is collinear: one segment per (fold, group)
    r = assert_equals_twin(ctx, "grid_one_ulp", 4)
    assert np.all(r["nseg"] == 2)                                    # ... but for the one point moved one ulp above the chord


def test_refusals(ctx):
    from chicdiff_amd.hip import ChicdiffHipError
    rng = np.random.default_rng(3)
    p, cov = rng.uniform(size=50), rng.uniform(size=50)

    def refused(match, p=p, cov=cov, **kw):
        args = dict(alpha=0.05, nbins=2, nfolds=3, seed=1)
        args.update(kw)
        with pytest.raises(ChicdiffHipError, match=match) as e:
            ctx.ihw_train(dev(ctx, p), dev(ctx, cov), **args)
        assert str(e.value).startswith("[1] ihw_train:")          # CHICDIFF_E_INVALID

    q = p.copy()
    q[17] = 1.5
    refused(r"pvalue\[17\] = 1\.5 is outside \[0, 1\]", p=q)
    q[17], q[31], q[40] = 0.5, -0.1, -0.2
    refused(r"pvalue\[31\] = -0\.1 is outside \[0, 1\]", p=q)
    cn = cov.copy()
    cn[23] = np.nan
    refused(r"covariate\[23\] is NaN on a kept row", cov=cn)
    q = p.copy()
    q[23] = np.nan                                                   # ... but not on a row that is left out
    assert ctx.ihw_train(dev(ctx, q), dev(ctx, cn), nbins=2, nfolds=3, seed=1)["m"] == 49
    refused("no kept row", p=np.full(50, np.nan))
    refused(r"nbins = 51 exceeds the 50 kept rows", nbins=51)
    refused(r"nbins = 257 .*256", nbins=257)
    refused(r"nfolds = 1 \(2 <= nfolds <= 16\)", nfolds=1)
    refused(r"nfolds = 17 \(2 <= nfolds <= 16\)", nfolds=17)
    for a in (0.0, 1.0, -0.5, float("nan")):
        refused(r"alpha = .* \(0 < alpha < 1\)", alpha=a)
    refused("chunk length 5 is not one of", chunk_len=5)
    r = ctx.ihw_train(dev(ctx, p), dev(ctx, cov), nbins=2, nfolds=3, seed=1)    # the context still works
    assert r["m"] == 50


def test_ihwcorrection_mirror_and_repeatable_pipeline(ctx, tmp_path):
    """IHWcorrection with the device trainer equals IHWcorrection with the twin as the trainer, in every column; the whole pipeline
    with the device trainer and a control seed gives the same table twice."""
    import pandas as pd
    from chicdiff_amd import pipeline
    from pipeline_inputs import make_experiment, read_chicago_pickle
    settings, _ = make_experiment(tmp_path, npeaks=1200, with_chinput=True)
    seen = {}
    real = pipeline.IHWcorrection

    def spy(*a, **kw):
        seen["args"], seen["kw"] = a, dict(kw)
        return real(*a, **kw)

    pipeline.IHWcorrection = spy
    try:
        run = lambda: pipeline.chicdiffPipeline(settings, ctx=ctx, read_chicago=read_chicago_pickle, ihw=pipeline.ihw_device(ctx, 5, nbins=5),
                                                rng=np.random.default_rng(11), control_seed=7)
        a, b = run(), run()
    finally:
        pipeline.IHWcorrection = real
    pd.testing.assert_frame_equal(a, b, check_exact=True)
    assert len(a) > 100 and a["weighted_padj"].notna().any()
    kw = dict(seen["kw"])
    kw["rng"], kw["ihw"] = np.random.default_rng(3), pipeline.ihw_device(ctx, 5, nbins=5)
    on_device = real(*seen["args"], **kw)
    kw["rng"], kw["ihw"] = np.random.default_rng(3), tw.ihw_callable(5, nbins=5)
    by_twin = real(*seen["args"], **kw)
    pd.testing.assert_frame_equal(on_device, by_twin, check_exact=True)
    with pytest.raises(ValueError, match="the trained weights are required"):
        kw["ihw"] = None
        real(*seen["args"], **kw)


def test_monotone_sanity_logged(ctx):
    """Logged, not asserted: 20 011 rows whose signal density falls with the covariate, 10 bins — the fold-averaged weights, and the
    rejections of weighted BH beside plain BH at 0.05."""
    k = ii.cases()["n20011"]
    dp, dc = dev(ctx, k["p"]), dev(ctx, k["cov"])
    r = ctx.ihw_train(dp, dc, alpha=0.05, nbins=10, nfolds=5, seed=k["seed"])
    g, f = r["group"].cpu().numpy(), r["fold"].cpu().numpy()
    w = r["weights"][g - 1, f]
    wp = np.where(w > 0, k["p"] / np.where(w > 0, w, 1.0), 1.0)
    plain = (ctx.bh_adjust(dp).cpu().numpy() <= 0.05).sum()
    weighted = (ctx.bh_adjust(dev(ctx, wp)).cpu().numpy() <= 0.05).sum()
    print("fold-averaged weights by group:", np.round(r["weights"].mean(axis=1), 3).tolist())
    print(f"rejections at 0.05: weighted BH {int(weighted)}, plain BH {int(plain)}")
