"""The twin of the region stage (tests/region_twin.py) and its inputs (tests/region_inputs.py), without a GPU:

  * chicdiff_amd/csrc/ru_window.h on its own (tests/region_window_host.cpp, built here with the C++ compiler) equals the window in Python
    integers on the whole grid of extreme IDs, and under the sanitisers;
  * every case reaches what it is for;
  * the numpy forms of the twin equal the statement-by-statement forms on every small case;
  * the CPU oracle equals the twin on all of them;
  * data.table's long-double mean equals the correctly rounded one on every avDist input used.

tests/test_gpu_region.py holds the device to the same twin on the same cases.
"""
import os
import shutil
import subprocess

import numpy as np
import pytest

import region_inputs as ri
import region_twin as rt
from post_inputs import region_universe_literal

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RU_KEYS = ("region_ptr", "baitID", "regionID", "otherEndID", "minOE", "maxOE")
RU_MAX_FRAG = 2 ** 30 - 1   # cd::kRuMaxFrag


def same_bits(a, b):
    a, b = np.ascontiguousarray(a, dtype=np.float64), np.ascontiguousarray(b, dtype=np.float64)
    nan = np.isnan(a)
    return a.shape == b.shape and np.array_equal(nan, np.isnan(b)) and np.array_equal(a[~nan].view(np.uint64), b[~nan].view(np.uint64))


@pytest.fixture(scope="module")
def oracle():
    from oracle import oracle as o
    o.build()
    return o


# ---- the header on its own ----------------------------------------------------------------------------------------------------
def grid_ids(maxfrag):
    return (list(range(ri.INT32_MIN, ri.INT32_MIN + 41)) + list(range(-41, 42)) + list(range(maxfrag - 41, maxfrag + 42))
            + list(range(ri.INT32_MAX - 40, ri.INT32_MAX + 1)))


GRID_S = (0, 1, 5, 15, 16, 17, 20, 40, 2 ** 20)


def expected_window_lines(maxfrag):
    ids, out = grid_ids(maxfrag), []
    for b in ids:
        for o in ids:
            for s in GRID_S:
                w = rt.window(b, o, s, maxfrag)
                lo, hi = w if w is not None else (1, 0)
                assert hi - lo + 1 <= max(2 * s + 1, 2)
                out.append(b"%d %d %d" % (lo, hi, 1 if w is None else 0))
    return out


def build_window_host(tmp_path, name, flags):
    cxx = shutil.which("g++") or shutil.which("c++") or shutil.which("clang++") or "/opt/rocm/llvm/bin/clang++"
    exe = str(tmp_path / name)
    subprocess.run([cxx, "-std=c++17", *flags, "-I", os.path.join(ROOT, "chicdiff_amd", "csrc"), os.path.join(ROOT, "tests", "region_window_host.cpp"),
                    "-o", exe], check=True)
    return exe


def window_lines(exe, maxfrag):
    return subprocess.run([exe, str(maxfrag)], capture_output=True, check=True).stdout.split(b"\n")[:-1]


def test_window_header_on_its_own_equals_python_integers(tmp_path):
    """ru_window.h is host and device code; this is its host half on every combination of the extreme IDs and RUexpand values (248 x 248
    x 9 per map size).  The program itself stops when a window holds more than max(2 s + 1, 2) IDs or leaves [1, maxfrag]."""
    exe = build_window_host(tmp_path, "region_window_host", ["-O2"])
    for maxfrag in (ri.MAXFRAG, 1, RU_MAX_FRAG):
        got, exp = window_lines(exe, maxfrag), expected_window_lines(maxfrag)
        assert len(got) == len(exp) == 248 * 248 * 9
        bad = [i for i, (g, e) in enumerate(zip(got, exp)) if g != e]
        assert not bad, (maxfrag, len(bad), bad[:5], [(got[i], exp[i]) for i in bad[:5]])
    assert subprocess.run([exe, str(RU_MAX_FRAG + 1)], capture_output=True).returncode == 2


def test_window_header_on_its_own_under_the_sanitisers(tmp_path):
    """The same stand-alone program built with -fsanitize=address,undefined (signed overflow is what it would report): host code in
    its own process."""
    exe = build_window_host(tmp_path, "region_window_host_san", ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"])
    assert window_lines(exe, ri.MAXFRAG) == expected_window_lines(ri.MAXFRAG)


# ---- the universe cases -------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def universe_twins():
    return [(c, rt.region_universe(c["bait"], c["oe"], c["s"], c["chr_of"])) for c in ri.universe_cases()]


def test_universe_cases_reach_what_they_are_for(universe_twins):
    seen = set()
    for c, t in universe_twins:
        s, chr_of, ln = c["s"], c["chr_of"], np.diff(t["region_ptr"])
        rows_of = lambda i: t["otherEndID"][t["region_ptr"][i]: t["region_ptr"][i + 1]].tolist()
        r_seq = lambda a, e: list(range(min(a, e), max(a, e) + 1))   # the set R's a:b holds, ascending
        width = lambda i: (lambda w: w[1] - w[0] + 1)(rt.window(c["bait"][i], c["oe"][i], s, ri.MAXFRAG))
        for name, rows in c["planted"].items():
            seen.add(name)
            for i in rows:
                b, o, got = int(c["bait"][i]), int(c["oe"][i]), rows_of(i)
                if name == "dist_s1_right":
                    assert o - b == s + 1 and got == r_seq(b + 2, o + s)
                elif name == "dist_s2_right":
                    assert o - b == s + 2 and got == list(range(o - s, o + s + 1)) and got[0] == b + 2
                elif name == "dist_s1_left":
                    assert b - o == s + 1 and got == r_seq(o - s, b - 2)
                elif name == "dist_s2_left":
                    assert b - o == s + 2 and got == list(range(o - s, o + s + 1)) and got[-1] == b - 2
                elif name == "beside_right":
                    assert got == ([b + 1, b + 2] if s == 0 else list(range(b + 2, o + s + 1)))   # R's descending (bait + 2):(oe + 0)
                elif name == "beside_left":
                    assert got == ([b - 2, b - 1] if s == 0 else list(range(o - s, b - 1)))
                elif name[0] == "w" and name[1:3].isdigit():
                    assert width(i) == int(name[1:3]) == len(got) and s >= 16   # beside windows of 2 s + 1 >= 33 candidates in the same launch
                elif name == "straddle_1":
                    assert got == list(range(max(1, o - s), o + s + 1)) and (s < 3 or got[0] == 1)
                elif name == "straddle_maxfrag":
                    assert got == list(range(o - s, min(o + s, ri.MAXFRAG) + 1)) and (s < 2 or got[-1] == ri.MAXFRAG)
                elif name == "straddle_chr":
                    assert got == list(range(o - s, min(o + s, ri.CHR_ENDS[0]) + 1)) and (s < 2 or len(got) < 2 * s + 1)
                elif name == "oe_other_chr":
                    assert got == list(range(o - s, ri.CHR_ENDS[0] + 1)) and chr_of[o] != chr_of[b]
                elif name == "hole_first":
                    assert chr_of[o - s] < 0 and (o - s) not in got and len(got) == 2 * s - (1 if s >= 10 else 0)
                elif name == "hole_last":
                    assert chr_of[o + s] < 0 and (o + s) not in got and len(got) == 2 * s - (1 if s >= 10 else 0)
                elif name == "hole_every":
                    assert got == [] and all(chr_of[x] < 0 for x in range(o - s, o + s + 1))
                elif name in ("bait_off_map", "bait_on_hole", "bait_zero", "bait_negative", "bait_above", "extreme", "empty_first", "empty_last",
                              "empty_run", "all_empty"):
                    assert got == []
                    if name.startswith("bait_") and name != "bait_zero" and name != "bait_negative":
                        assert width(i) > 0   # the window itself is on the map: it is the bait that empties the region
                else:
                    raise AssertionError(name)
        if "empty_run" in c["planted"]:
            assert len(c["planted"]["empty_run"]) >= 256 and c["planted"]["empty_run"][0] % 256 == 0 and ln[512] > 0 and ln[:256].sum() > 0
        if "all_empty" in c["planted"]:
            assert t["region_ptr"][-1] == 0
        if "extreme" in c["planted"] and len(c["bait"]) > 1:
            ids = set(c["bait"][c["planted"]["extreme"]].tolist()) | set(c["oe"][c["planted"]["extreme"]].tolist())
            assert set(ri.EXTREMES) <= ids
            assert all(ln[i - 1] > 0 or ln[i + 1] > 0 for i in c["planted"]["extreme"][:5])   # between normal peaks
        if s >= 16 and len(c["bait"]) > 1:
            widths = {width(i) for i in range(len(c["bait"]))}
            assert {31, 32, 33, 2 * s + 1} <= widths
        if s == 0 and len(c["bait"]) > 1:
            assert ln.max() == 2
        assert np.array_equal(t["minOE"] == rt.NA_INT, ln == 0) and np.array_equal(t["maxOE"] == rt.NA_INT, ln == 0)
    need = {"dist_s1_right", "dist_s2_right", "dist_s1_left", "dist_s2_left", "beside_right", "beside_left", "straddle_1", "straddle_maxfrag",
            "straddle_chr", "oe_other_chr", "hole_first", "hole_last", "hole_every", "bait_off_map", "bait_on_hole", "bait_zero", "bait_negative",
            "bait_above", "extreme", "empty_first", "empty_last", "empty_run", "all_empty"}
    need |= {f"w{w}_{where}" for w in (31, 32, 33) for where in ("near", "end", "start")}
    assert need <= seen, need - seen
    assert {len(c["bait"]) for c, _ in universe_twins} >= set(ri.UNIVERSE_N) and {c["s"] for c, _ in universe_twins} == set(ri.UNIVERSE_S)


def test_universe_numpy_form_equals_the_literal_form(universe_twins):
    for c, t in universe_twins:
        v = rt.region_universe_np(c["bait"], c["oe"], c["s"], c["chr_of"])
        for k in RU_KEYS:
            assert v[k].dtype == t[k].dtype and np.array_equal(v[k], t[k]), (len(c["bait"]), c["s"], k)
    for name, bait, oe, chr_of, s, row in ri.refusal_cases():
        for f in (rt.region_universe, rt.region_universe_np):
            with pytest.raises(ValueError, match="Invalid parameters"):
                f(bait, oe, s, chr_of)


def test_oracle_region_universe_equals_the_twin(oracle, universe_twins):
    """the repaired oracle_region_universe (64-bit window, clamped to the map) on every case, the extreme IDs among the rows"""
    for c, t in universe_twins:
        ptr, rb, rr, ro = oracle.region_universe(c["bait"], c["oe"], c["s"], c["chr_of"])
        for k, got in (("region_ptr", ptr), ("baitID", rb), ("regionID", rr), ("otherEndID", ro)):
            assert np.array_equal(got, t[k]), (len(c["bait"]), c["s"], k)
    for name, bait, oe, chr_of, s, row in ri.refusal_cases():
        with pytest.raises(ValueError, match="Invalid parameters"):
            oracle.region_universe(bait, oe, s, chr_of)


def test_oracle_region_universe_on_the_overflow_findings(oracle):
    """One peak on a map of 3 000 IDs on one chromosome.  With the window in 32-bit int, bait = 100, oe = 2147483645, RUexpand = 5 wrapped
    to (-2147483646 .. 2147483640): 3 000 rows after about 10^9 steps; bait = 100, oe = 2147483647, RUexpand = 0 never left the loop."""
    chr_of = np.zeros(3001, dtype=np.int32)
    chr_of[0] = -1
    for oe, s in ((2147483645, 5), (2147483647, 0), (-2147483648, 5), (-2147483644, 5)):
        b, o = np.array([100], np.int32), np.array([oe], np.int32)
        assert len(region_universe_literal(b, o, s, chr_of)) == 0
        ptr, rb, rr, ro = oracle.region_universe(b, o, s, chr_of)
        assert ptr.tolist() == [0, 0] and len(ro) == 0


def test_universe_stride_case_is_what_it_says():
    c = ri.universe_stride_case()
    assert len(c["bait"]) == 4096 * 256 + 1 and c["s"] == 5
    v = rt.region_universe_np(c["bait"][-2000:], c["oe"][-2000:], 5, c["chr_of"])
    assert np.diff(v["region_ptr"])[-1] > 0 and set(ri.EXTREMES) <= set(c["oe"].tolist())


# ---- key table ----------------------------------------------------------------------------------------------------------------
def test_key_table_cases_and_forms(oracle):
    seen = set()
    for c in ri.key_table_cases() + [ri.key_table_repeats()]:
        keys, vals = rt.key_table(c["bait"], c["oe"], c["N"], c["flags"])
        k2, v2 = rt.key_table_np(c["bait"], c["oe"], c["N"], c["flags"])
        assert np.array_equal(keys, k2) and np.array_equal(vals, v2) and keys.dtype == k2.dtype and vals.dtype == v2.dtype
        k3, v3 = oracle.count_table(c["bait"], c["oe"], c["N"], c["flags"])
        assert np.array_equal(keys, k3) and np.array_equal(vals, v3)
        assert np.all(np.diff(keys) >= 0) and np.all(keys >= 0)
        kept = set(zip(keys.tolist(), vals.tolist()))
        given, empty = c["flags"] is not None, c["flags"] is not None and not c["flags"].any()
        if empty:
            assert len(keys) == 0
        for name, rows in c["planted"].items():
            seen.add(name)
            b, o, v = int(c["bait"][rows[0]]), int(c["oe"][rows[0]]), int(c["N"][rows[0]])
            here = (rt.pack(b, o), v) in kept
            if name in ("bait_negative", "bait_int32_min"):
                assert b < 0 and not here
            elif name in ("bait_int32_max", "bait_int32_max_oe_negative", "bait_above_max_id"):
                assert b > ri.KEY_MAX_ID and here == (not given)
            elif name == "repeat":
                at = np.flatnonzero(keys == rt.pack(b, o))
                assert vals[at].tolist() == c["N"][rows].tolist() and len(at) == 3      # file order among equal keys
            else:
                assert here == (not empty)
                if name == "oe_negative" and here:                                        # behind every positive otherEndID of its bait
                    mine = keys[(keys >> 32) == b] & 0xFFFFFFFF
                    assert (mine > 0x7FFFFFFF).any() and np.all(np.diff(mine) > 0)
    assert seen >= {"oe_negative", "bait_negative", "bait_int32_max", "oe_int32_min", "oe_int32_max", "N_zero", "N_negative", "N_int32_max",
                    "bait_int32_min", "bait_above_max_id", "repeat"}


def test_key_table_stride_case_numpy_form():
    c = ri.key_table_case(ri.KEY_STRIDE_ROWS, "given")
    keys, vals = rt.key_table_np(c["bait"], c["oe"], c["N"], c["flags"])
    assert len(c["bait"]) == 2048 * 2048 + 1 and 0 < len(keys) < len(c["bait"]) and np.all(np.diff(keys) > 0)


# ---- joins --------------------------------------------------------------------------------------------------------------------
def test_join_cases_reach_what_they_are_for_and_the_oracle_agrees(oracle):
    seen, shapes = set(), set()
    for c in ri.join_cases():
        S, dicts = c["S"], c["dicts"]
        for (keys, vals), d in zip(c["tables"], dicts):
            assert rt.table_dict(keys, vals) == d and np.all(np.diff(keys) > 0)
        inner = rt.join_inner(c["qbait"], c["qoe"], dicts)
        left = [rt.join_left(c["qbait"], c["qoe"], d) for d in dicts]
        assert np.array_equal(oracle.count_join_inner(c["qbait"], c["qoe"], c["tables"]), inner)
        for (keys, vals), exp in zip(c["tables"], left):
            assert np.array_equal(oracle.count_join(c["qbait"], c["qoe"], keys, vals), exp)
        shapes.add((S, len(c["qbait"])))
        if c["variant"] == "one_empty":
            assert not inner.any() and any(len(k) == 0 for k, _ in c["tables"]) and (S == 1 or any(x.any() for x in left))
            seen.add("one_empty")
        if c["variant"] == "one_key":
            assert all(len(k) == 1 for k, _ in c["tables"])
        for name, rows in c["planted"].items():
            for r in rows:
                q = (int(c["qbait"][r]), int(c["qoe"][r]))
                if c["variant"] == "one_key":
                    if name == "one_key":
                        assert inner[r].tolist() == [t + 1 for t in range(S)]
                    else:
                        assert not inner[r].any()
                        only = rt.pack(5, 9)
                        if name in ("below", "above"):
                            key = (q[0] << 32) | (q[1] & 0xFFFFFFFF)
                            assert (key < only) if name == "below" else (key > only)
                    seen.add("one_key:" + name)
                    continue
                if c["variant"] != "normal":
                    continue
                seen.add(name)
                if name in ("first", "last"):
                    assert all((k[0] if name == "first" else k[-1]) == rt.pack(*q) for k, _ in c["tables"]) and inner[r].all()
                elif name == "zero_hit":
                    assert inner[r, 0] == 0 and (S == 1 or inner[r, 1:].all()) and all(q in d for d in dicts)
                elif name.startswith("all_but_"):
                    missing = {"all_but_first": 0, "all_but_middle": S // 2, "all_but_last": S - 1}[name]
                    assert [q in d for d in dicts] == [t != missing for t in range(S)] and not inner[r].any()
                    assert S == 1 or any(x[r] for x in left)     # the plain join still finds it in the other tables
                elif name in ("below", "above"):
                    key = (q[0] << 32) | (q[1] & 0xFFFFFFFF)
                    assert all((key < k[0]) if name == "below" else (key > k[-1]) for k, _ in c["tables"]) and not inner[r].any()
                elif name in ("between", "one_key"):
                    pass
                else:
                    raise AssertionError(name)
        if c["variant"] == "normal" and len(c["qbait"]) >= 255:
            hit = inner.any(axis=1).mean()
            assert 0 < hit < 1 or S == 64   # with 64 tables at 80 % hardly any random pair is in all of them: the planted ones are
            assert inner.any()
    assert shapes >= {(S, n) for S in ri.JOIN_S for n in ri.JOIN_NRU}
    assert seen >= {"first", "last", "zero_hit", "all_but_first", "all_but_middle", "all_but_last", "below", "above", "one_empty", "one_key:one_key",
                    "one_key:below", "one_key:above"}, seen
    assert any(int(c["qbait"][r]) < 0 for c in ri.join_cases() for r in c["planted"].get("below", []))


# ---- avDist -------------------------------------------------------------------------------------------------------------------
def test_avdist_cases_long_double_mean_and_the_oracle(oracle):
    midsum, chr_codes = ri.avdist_map()
    odd = midsum[midsum % 2 == 1]
    assert (odd % 4 == 1).any() and (odd % 4 == 3).any() and midsum.max() // 2 > 4.9e8          # both half-to-even directions; large midpoints
    mids = {int(m): round(__import__("fractions").Fraction(int(m), 2)) for m in odd[:8].tolist()}
    assert all(v % 2 == 0 and abs(2 * v - m) == 1 for m, v in mids.items()) and {2 * v - m for m, v in mids.items()} == {1, -1}
    assert (chr_codes < 0).any()
    seen = set()
    for c in ri.avdist_cases():
        args = (c["ru_bait"], c["ru_oe"], c["region_ptr"], c["id_min"], c["midsum"], c["chr"])
        exact, ld = rt.avdist(*args), rt.avdist_long_double(*args)
        assert same_bits(exact, ld)                                    # every region below 1 024 rows: the two routes agree
        assert same_bits(oracle.region_avdist(*args), exact)
        assert np.diff(c["region_ptr"]).max() < 1024
        nochr = rt.avdist(*args[:5], None)
        for kind, rows in c["planted"].items():
            seen.add((kind, c["chr"] is not None))
            v = exact[rows]
            if kind in ("empty", "off_map_all"):
                assert np.isnan(v).all()
            elif kind == "trans":
                assert np.isnan(v).all() == (c["chr"] is not None) and not np.isnan(nochr[rows]).any()
            elif kind == "negative_code":
                assert not np.isnan(v).any() and (c["chr"] is None or not np.array_equal(v, nochr[rows]))
            else:
                assert not np.isnan(v).any()
        ok = exact[~np.isnan(exact)]
        if len(ok) > 20:
            assert (ok < 0).any() and (ok > 0).any() and (ok != np.round(ok)).any()
    assert seen == {(k, w) for k in ri.AV_KINDS for w in (False, True)}
    assert {len(c["region_ptr"]) - 1 for c in ri.avdist_cases()} == set(ri.AVDIST_N)
