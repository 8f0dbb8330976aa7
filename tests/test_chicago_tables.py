"""The Chicago background tables on the device (chicdiff_hip_chicago_tables_dev, chicdiff.R:656-692, 538-548): what can be checked
without a GPU — the declaration, the code preparation and the split distance function against the host twin
(pipeline.background_tables), and that the adversarial tables of tests/chicago_tables_inputs.py tell a right winner from a wrong one.
The device itself is compared with the twin in tests/test_chicago_tables_gpu.py."""
import inspect
import os
import re
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import chicago_tables_inputs as cti  # noqa: E402


def test_declared_cited_exported():
    import __graft_entry__ as g
    g.build()
    from chicdiff_amd import hip, pipeline
    sym = "chicdiff_hip_chicago_tables_dev"
    hdr = open(os.path.join(ROOT, "include", "chicdiff_hip.h")).read()
    k = hdr.index("int " + sym + "(")
    comment = hdr[hdr.rindex("/*", 0, hdr.rindex("*/", 0, k)):k]
    assert "656-692" in comment and "538-548" in comment and "(baitID, otherEndID, r)" in comment
    assert sym in hip.EXPORTS and hasattr(hip.load_library(), sym)
    assert callable(hip.HipContext.chicago_tables)
    caps = hip.chicago_tables_caps()
    for name, key in (("CHICDIFF_CHICAGO_MAX_PAIRS", "max_pairs"), ("CHICDIFF_CHICAGO_MAX_DISTBIN", "max_distbin"),
                      ("CHICDIFF_CHICAGO_ROWS_PER_WORKGROUP", "rows_per_workgroup")):
        assert int(re.search(r"#define\s+" + name + r"\s+(\d+)", hdr).group(1)) == caps[key] > 0
    mk = open(os.path.join(ROOT, "chicdiff_amd", "csrc", "Makefile")).read()
    assert "chicago_kernels.hip" in re.search(r"^SRCS\s*:=(.*)$", mk, re.M).group(1)
    assert inspect.signature(pipeline.getFullRegionData).parameters["device_tables"].default is False
    assert list(inspect.signature(pipeline.background_tables_dev).parameters)[:4] == ["xs", "id_min", "nid", "ctx"]
    assert list(inspect.signature(pipeline.chicEstimateDistFun).parameters) == ["x", "binsize"]


@pytest.mark.parametrize("categorical", [False, True], ids=["strings", "categoricals"])
def test_codes_follow_the_twins_levels(categorical):
    """chicago_codes returns background_tables' levB / levL, and every row's code names the row's own label — for string columns and
    for pandas categoricals (one of them with its categories in another order and a category that no row shows)."""
    from chicdiff_amd import pipeline
    xs = [cti.table(4097, 1), cti.table(65, 2), cti.table(64, 3)]
    xs[2] = xs[2][xs[2]["tblb"] != cti.LEVB[0]].reset_index(drop=True)    # a replicate that lacks a level
    nid = cti.nid_of(4097)
    twin = pipeline.background_tables(xs, cti.ID_MIN, nid)
    if categorical:
        import pandas as pd
        xs = [x.copy() for x in xs]
        for j, x in enumerate(xs):
            for col, lev in (("tblb", cti.LEVB), ("tlb", cti.LEVL)):
                cats = (lev + ["(never,seen]"])[::-1] if j == 1 else lev
                x[col] = pd.Categorical(x[col], categories=cats)
            x["distbin"] = pd.Categorical(x["distbin"])
        twin_cat = pipeline.background_tables(xs, cti.ID_MIN, nid)
        assert twin_cat["levB"] == twin["levB"] and twin_cat["levL"] == twin["levL"]
    cd = pipeline.chicago_codes(xs)
    assert cd["levB"] == twin["levB"] == sorted(cti.LEVB) and cd["levL"] == twin["levL"] == sorted(cti.LEVL)
    for s, x in enumerate(xs):
        for col, lev in (("tblb", cd["levB"]), ("tlb", cd["levL"])):
            c = cd[col][s]
            assert c.dtype == np.int32 and c.shape == (len(x),)
            want = np.array([lev.index(str(v)) if v == v and v is not None else -1 for v in x[col]])
            assert np.array_equal(c, want), (s, col)
        d, labels = cd["distbin"][s], x["distbin"].to_numpy(dtype=object)
        assert d.dtype == np.int32 and d.min() == -1 and d.max() < cd["ndistbin"][s]
        assert np.array_equal(d < 0, np.array([v is None or v != v for v in labels]))
        seen = {}
        for code, v in zip(d, labels):                                  # one code per label and one label per code
            if code >= 0:
                assert seen.setdefault(int(code), v) == v
        assert len(set(seen.values())) == len(seen)


def test_distance_function_from_values(tmp_path):
    """chicEstimateDistFunValues on the multiset of the issue's definition — refBinMean over the distinct (distbin, refBinMean) pairs
    with a non-NA refBinMean, an NA distbin counting as a value, sorted descending — gives chicEstimateDistFun's ten numbers, bit for bit."""
    from chicdiff_amd import pipeline
    from pipeline_inputs import make_experiment
    _, truth = make_experiment(tmp_path, npeaks=300)
    for x in truth["xs"] + [cti.table(4097, 1), cti.table(20011, 1, True)]:
        pairs = {(None if d is None or d != d else d, float(v)) for d, v in zip(x["distbin"], x["refBinMean"]) if v == v}
        values = np.sort(np.array([v for _, v in pairs]))[::-1]
        assert len(values) >= 4
        got, want = pipeline.chicEstimateDistFunValues(values), pipeline.chicEstimateDistFun(x)
        assert got.shape == (10,) and np.array_equal(got.view(np.int64), want.view(np.int64))


@pytest.mark.parametrize("n,dups", [(4097, False), (20011, True)])
def test_generator_tells_first_from_last(n, dups):
    """On the adversarial tables the twin with "first" replaced by "last" differs in more than half of the seen baits' sj and of
    the seen other ends' si: a device that picked any row of a group would not pass the parity tests."""
    from chicdiff_amd import pipeline
    x, nid = cti.table(n, 1, dups), cti.nid_of(n)
    first = pipeline.background_tables([x], cti.ID_MIN, nid)
    last = cti.twin_keeping("last")([x], cti.ID_MIN, nid)
    again = cti.twin_keeping("first")([x], cti.ID_MIN, nid)
    for k in ("sj", "si", "T", "distfun"):
        assert cti.same_bits(first[k], again[k]), k
    for col, k in (("baitID", "sj"), ("otherEndID", "si")):
        ids = np.unique(x[col].to_numpy())
        ids = ids[(ids >= cti.ID_MIN) & (ids < cti.ID_MIN + nid)] - cti.ID_MIN
        a, b = first[k][0, ids], last[k][0, ids]
        differ = ~((a == b) | (np.isnan(a) & np.isnan(b)))
        assert differ.mean() > 0.5, (k, differ.mean())
    assert not cti.same_bits(first["T"], last["T"])
