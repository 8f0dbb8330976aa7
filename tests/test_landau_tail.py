"""landau_tail (devmath.h), the Landau tail Q(z) behind getCandidateInteractions(method = "hmp"), without a GPU: the numpy twin of
the committed coefficients (tests/hmp_twin.py) against tests/golden/landau_tail.json (mpmath, tools/make_landau_golden.py).

Errors are counted in units u(z) = 2^-52 Q(z) max(1, (1 + |z|) |d log Q / dz|): the relative rounding unit, scaled by the
function's own conditioning in z, because z arrives rounded.  The twin's largest error over the golden abscissae, measured
here, is hmp_twin.LANDAU_TWIN_MAX_UNITS (profiles/r19_landau_accuracy.json, "twin"); the bound asserted, here and for the device
(test_landau_tail_gpu.py), is that figure doubled and rounded up to a whole unit, as DELTA_BOUND_UNITS is."""
import inspect
import json
import math
import os
import re
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import hmp_twin as ht  # noqa: E402


golden, error_units, record = ht.golden, ht.error_units, ht.record


def test_bound_follows_the_twins_measured_figure():
    assert ht.LANDAU_BOUND_UNITS == math.ceil(2 * ht.LANDAU_TWIN_MAX_UNITS)


def test_twin_against_golden():
    g, z = golden()
    assert 1800 <= len(z) <= 2200 and z.min() == -14.0 and z.max() == math.inf and 2.0 ** 1023 in z
    err = error_units(z, ht.landau_tail_twin(z), g)
    k = int(np.argmax(err))
    print(f"twin: off by at most {err[k]:.3f} units, at z = {z[k]!r}")
    record("twin", float(err[k]), z[k])
    assert err[k] <= ht.LANDAU_BOUND_UNITS


def test_golden_holds_every_seam_and_the_cut_over():
    _, z = golden()
    t = ht.load_table()
    have = set(z.tolist())
    for b in ht.table_bounds(t):
        assert {math.nextafter(b, -math.inf), b, math.nextafter(b, math.inf)} <= have, b
    assert ht.table_bounds(t)[-1] == t["cut"]


def test_monotone_across_goldens_and_seams():
    _, z = golden()
    q = ht.landau_tail_twin(np.sort(z))
    assert (np.diff(q) <= 0).all()
    for b in ht.table_bounds(ht.load_table()):
        lo, at, hi = ht.landau_tail_twin([math.nextafter(b, -math.inf), b, math.nextafter(b, math.inf)])
        assert lo >= at >= hi, b


def test_ends_and_range():
    q = ht.landau_tail_twin
    assert (q([-14.0, -14.5, -1e300, -math.inf, -3.5]) == 1.0).all()
    assert q(math.inf)[0] == 0.0 and np.isnan(q(math.nan)[0])
    rng = np.random.default_rng(19)
    z = np.concatenate([rng.uniform(-14, 140, 20000), np.exp(rng.uniform(0, 709, 5000)), -np.exp(rng.uniform(-40, 3, 2000))])
    v = q(z)
    assert (v <= 1.0).all() and (v >= 0.0).all() and not np.isnan(v).any()


def test_table1_of_the_paper():
    g, _ = golden()
    assert [r["L"] for r in g["table1"]] == [10, 100, 1000, 10000]
    for r in g["table1"]:
        z = (1.0 / r["threshold"] - (math.log(r["L"]) + ht.HMP_LOC)) / ht.HMP_SCALE
        v = float(ht.landau_tail_twin(z)[0])
        assert abs(v - float(r["tail"])) < 1e-6 and round(v, 2) == r["expected"] == 0.05, (r, v)


def test_declared_cited_exported():
    import __graft_entry__ as g
    g.build()
    from chicdiff_amd import hip
    hdr = open(os.path.join(ROOT, "include", "chicdiff_hip.h")).read()
    k = hdr.index("int chicdiff_hip_candidate_interactions_method_dev(")
    comment = hdr[hdr.rindex("/*", 0, k):k]
    assert "2135-2137, 2146" in comment and "unpinned" in comment and "mpmath" in comment and "FMStable" in comment
    assert "#define CHICDIFF_CAND_MIN 0" in comment and "#define CHICDIFF_CAND_HMP 1" in comment
    old = hdr.index("int chicdiff_hip_candidate_interactions_dev(")
    assert "not offered" not in hdr[hdr.rindex("/*", 0, old):old]
    assert "int chicdiff_hip_selftest_landau_dev(" in hdr
    lib = hip.load_library()
    for name in ("chicdiff_hip_candidate_interactions_method_dev", "chicdiff_hip_selftest_landau_dev"):
        assert name in hip.EXPORTS and hasattr(lib, name) and getattr(lib, name).argtypes
    assert len(lib.chicdiff_hip_candidate_interactions_method_dev.argtypes) == len(lib.chicdiff_hip_candidate_interactions_dev.argtypes) + 1
    sig = inspect.signature(hip.HipContext.candidate_interactions)
    assert sig.parameters["method"].default == "min" and hip.CAND_METHODS == {"min": 0, "hmp": 1}
    assert callable(hip.HipContext.selftest_landau)
    src = open(os.path.join(ROOT, "chicdiff_amd", "csrc", "candidate_kernels.hip")).read()
    assert re.search(r"template <int METHOD>\s*__global__ __launch_bounds__\(256\) void cand_overlap_kernel", src)
    assert "__shared__" not in open(os.path.join(ROOT, "chicdiff_amd", "csrc", "devmath.h")).read().split("struct LandauTable")[1]


def test_hmp_without_a_context_names_the_opt_in():
    import pytest
    from chicdiff_amd import pipeline
    with pytest.raises(ValueError, match=r"harmonicmeanp::p\.hmp.*HipContext"):
        pipeline.getCandidateInteractions(None, None, {}, method="hmp", ctx=None)
