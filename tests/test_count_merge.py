"""chicdiff_hip_count_tables_merge_dev without a GPU: the entry point is declared, listed and exported, the keywords exist and are off,
and the theorem the call rests on holds on the project's own join cases — with the twin of tests/region_twin.py alone (dicts and Python
integers): the LEFT join against the merged tables (mergedFiles <- Reduce(merge, tempForCounts), chicdiff.R:778) is the INNER join of
the branch without chinput files (:774-807) against the original ones, on every query.  Every comparison is an equality."""
import inspect
import os
import re

import numpy as np
import pytest

import region_inputs as ri
import region_twin as rt

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYM = "chicdiff_hip_count_tables_merge_dev"


def merged_tables(dicts):
    """Reduce(merge) by the twin, as the device returns it: the kept pairs sorted by ``pack`` (one key column) and one value column per
    replicate -> (keys int64, vals (S, n) int32, the merged tables as dicts)."""
    pairs = sorted(rt.reduce_merge(dicts), key=lambda p: rt.pack(*p))
    keys = np.array([rt.pack(*p) for p in pairs], dtype=np.int64).reshape(-1)
    vals = np.array([[d[p] for p in pairs] for d in dicts], dtype=np.int32).reshape(len(dicts), len(pairs))
    return keys, vals, [{p: d[p] for p in pairs} for d in dicts]


def test_entry_point_is_declared_listed_and_exported():
    import __graft_entry__ as g
    g.build()
    from chicdiff_amd import hip, pipeline
    hdr = open(os.path.join(ROOT, "include", "chicdiff_hip.h")).read()
    assert re.search(r"\bint\s+" + SYM + r"\s*\(", hdr)
    rule = hdr[hdr.index("the merge alone"):hdr.index("int " + SYM)]
    for lines in (":778", "774-807", "1202-1260"):                    # the reference lines it states
        assert lines in rule, lines
    assert "bit for bit" in rule and "Reduce(merge" in rule and "ascending and unique" in rule and "overlap" in rule
    assert "NOT covered" not in hdr and SYM in hdr[hdr.index("a1 + a3 + a2"):hdr.index("int chicdiff_hip_region_assemble_dev")]
    assert SYM in hip.EXPORTS and hasattr(hip.load_library(), SYM)
    assert hasattr(hip.HipContext, "merge_count_tables")
    for f in (pipeline.getFullRegionData, pipeline.chicdiffPipeline):
        assert inspect.signature(f).parameters["merge_counts"].default is False


def test_assemble_without_count_data_names_the_keyword(tmp_path):
    from chicdiff_amd import pipeline
    from pipeline_inputs import make_experiment
    settings, _ = make_experiment(tmp_path, npeaks=300, with_chinput=False)
    with pytest.raises(ValueError, match="merge_counts=True"):
        pipeline.getFullRegionData(settings, None, None, ctx=None, read_chicago=lambda p: None, assemble=True)


@pytest.mark.parametrize("c", ri.join_cases(), ids=lambda c: f"S{c['S']}-nru{len(c['qbait'])}-{c['variant']}")
def test_left_join_of_the_merged_tables_is_the_inner_join(c):
    keys, vals, merged = merged_tables(c["dicts"])
    assert np.all(keys[1:] > keys[:-1])
    inner = rt.join_inner(c["qbait"], c["qoe"], c["dicts"])           # (nru, S)
    for s, m in enumerate(merged):
        assert rt.table_dict(keys, vals[s]) == m
        assert np.array_equal(rt.join_left(c["qbait"], c["qoe"], m), inner[:, s]), s
    # the whole key space of the case, not only its queries: every pair any table holds
    pairs = sorted(set().union(*c["dicts"]))
    if pairs:
        b, o = [p[0] for p in pairs], [p[1] for p in pairs]
        inner = rt.join_inner(b, o, c["dicts"])
        for s, m in enumerate(merged):
            assert np.array_equal(rt.join_left(b, o, m), inner[:, s]), s


def test_a_pair_with_a_zero_count_is_held():
    """"zero_hit" (held by all, N = 0 in table 0) is IN the merged table; reading a hit as ``value != 0`` loses it."""
    c = ri.join_case(3, 257)
    zero = (10, 300)
    assert all(zero in d for d in c["dicts"]) and c["dicts"][0][zero] == 0 and c["dicts"][1][zero] != 0
    keys, vals, merged = merged_tables(c["dicts"])
    at = int(np.searchsorted(keys, rt.pack(*zero)))
    assert keys[at] == rt.pack(*zero) and vals[:, at].tolist() == [d[zero] for d in c["dicts"]]
    by_value = set(c["dicts"][0])
    for d in c["dicts"]:
        by_value &= {p for p, v in d.items() if v != 0}               # the wrong reading: "absent" where the count is 0
    assert zero not in by_value and by_value != rt.reduce_merge(c["dicts"])
    wrong = [{p: d[p] for p in by_value} for d in c["dicts"]]
    rows = c["planted"]["zero_hit"]
    inner = rt.join_inner(c["qbait"], c["qoe"], c["dicts"])
    assert (inner[rows, 1] != 0).all()
    assert not np.array_equal(rt.join_left(c["qbait"], c["qoe"], wrong[1]), inner[:, 1])
    assert np.array_equal(rt.join_left(c["qbait"], c["qoe"], merged[1]), inner[:, 1])
