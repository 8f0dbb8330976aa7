""".multimerge without a GPU (chicdiff.R:218-228, 234-236): the plain-Python twin of the rule above chicdiff_hip_peaks_textkeys_dev in
include/chicdiff_hip.h (tests/peaks_merge_twin.py) against pandas — the classifier against pandas' own typing, the merged and filtered
table against readAndFilterPeakMatrix([files...]) on the host, the decline cases against what the host gives — and the library's host
statement of the text keys against the twin.  tests/test_peaks_merge_gpu.py holds the device to the twin."""
import io
import os
import re
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import peaks_merge_inputs as mi  # noqa: E402
import peaks_merge_twin as mt  # noqa: E402
import peaks_twin as tw  # noqa: E402


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.int64)


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as g
    g.build()
    from chicdiff_amd import hip
    return hip


# ---- the classifier against pandas' typing ---------------------------------------------------------------------------------------------
TOKENS = (["01", "+1", "1.0", "1e5", "2L", "inf", "-", "1_0", "0x10", "Inf", "+inf", "-INF", "infinity", "-Infinity", "+infinity", "INFINITY"]
          + [t.decode() for t in mt.NA_SPELLINGS if t]
          + ["0", "1", "7", "19", "10", "123456789", "999999999", "1234567890", "007", "-1", "-0", "1.", ".5", "1e", "e", "E", "+", ".", "e5",
             "X", "chrX", "chr1", "chr10_gl", "abcdefgh", "abcdefghi", "chr1_random", "MT", "2R", "True", "a b", "1 ", " 1", "café", "é",
             "NAN", "na", "Nan", "#N/A!", "N/A N/A", "1.#INF", "x" * 8, "x" * 9, "1" * 8 + "x", "1" * 7 + "x"])


@pytest.mark.parametrize("tok", TOKENS, ids=[repr(t) for t in TOKENS])
def test_classifier_agrees_with_pandas_typing(tok):
    """A two-row column, the token beside 1, through the python engine: int64 with the value unchanged means plain integer, object
    with the strings unchanged means text, and anything else must be declined."""
    import pandas as pd
    kind = mt.classify(tok.encode())
    col = pd.read_csv(io.StringIO(f"a\tb\n{tok}\t0\n1\t0\n"), sep="\t", engine="python")["a"]
    if col.dtype == np.int64 and str(col[0]) == tok:
        pandas_kind = "int"
    elif col.dtype == object and col.tolist() == [tok, "1"]:
        pandas_kind = "text"
    else:
        pandas_kind = "declined"
    if kind == "int":
        assert pandas_kind == "int" and int(tok) == col[0]
    elif kind == "text":
        assert pandas_kind == "text" and len(tok.encode()) <= 8
    else:
        assert kind in ("long", "ambiguous")                                     # (declining what pandas would type is allowed)
    if pandas_kind == "declined":
        assert kind in ("long", "ambiguous"), (tok, col.dtype, col.tolist())


def test_classifier_on_the_named_cases():
    want = {"01": "ambiguous", "+1": "ambiguous", "1.0": "ambiguous", "1e5": "ambiguous", "inf": "ambiguous", "-": "ambiguous", "": "ambiguous",
            "2L": "text", "1_0": "text", "0x10": "text", "abcdefgh": "text", "abcdefghi": "long", "café": "ambiguous", "0": "int",
            "123456789": "int", "1234567890": "ambiguous", "+infinity": "long", "Infinity": "ambiguous"}
    for t in mt.NA_SPELLINGS:
        want[t.decode()] = "ambiguous"
    for tok, kind in want.items():
        assert mt.classify(tok.encode()) == kind, tok


def test_text_key_order_is_str_order():
    rng = np.random.default_rng(3)
    alphabet = "0123456789ABXYZabcxyz_.-+~!"
    toks = {"".join(rng.choice(list(alphabet), int(rng.integers(1, 9)))) for _ in range(4000)} | {"1", "10", "2", "X", "chr1", "chr10", "chr2", "chr1_"}
    toks = sorted(toks)                                                         # Python's str order (ASCII: code points are bytes)
    keys = [mt.text_key(t.encode()) for t in toks]
    assert keys == sorted(keys) and len(set(keys)) == len(keys)
    assert all(-(1 << 63) <= k < (1 << 63) for k in keys)
    assert mt.text_key(b"10") < mt.text_key(b"2") < mt.text_key(b"X")
    cls, status, k = mt.column_keys([b"1", b"2L", b"10"])
    assert (cls, status) == (mt.KEY_MIXED, 0) and k == [mt.text_key(b"1"), mt.text_key(b"2L"), mt.text_key(b"10")]
    assert mt.column_keys([b"3", b"10"]) == (mt.KEY_INT, 0, [3, 10])
    assert mt.column_keys([b"123456789", b"X"])[1] == mt.ST_CHR_LONG             # a 9-digit number has no 8-byte key


# ---- the merge twin against the host path -----------------------------------------------------------------------------------------------
def same_as_host(paths, chicago, targets, tmp_path, tag):
    """The twin's merged and filtered table against readAndFilterPeakMatrix on the host: rows, order, every column, _filteredBaits.txt."""
    from chicdiff_amd import pipeline
    assert mt.decline(paths, targets) is None, tag
    t = mt.read_and_filter(paths, targets, chicago, mi.SCORE)
    x = pipeline.readAndFilterPeakMatrix(paths, targets, chicago, list(chicago), mi.SCORE, outprefix=str(tmp_path / "host"))
    assert list(x.columns) == mi.KEYS + t["names"], tag
    assert len(x) == len(t["kept"]), tag
    want = open(str(tmp_path / "host") + "_filteredBaits.txt", "rb").read()
    assert "".join(f"{b}\n" for b in t["filtered"]).encode() == want, tag
    for c in x.columns:
        got = t["columns"][c]
        if c in ("baitChr", "baitName", "oeChr", "oeName"):
            assert list(got) == x[c].astype(str).tolist(), (tag, c)
        elif c == "dist" or c in t["names"]:
            assert np.array_equal(bits(got), bits(x[c].to_numpy(np.float64))), (tag, c)   # 6-digit tokens: both readers give float(token)
        else:
            assert np.array_equal(np.asarray(got, dtype=np.int64), x[c].to_numpy(np.int64)), (tag, c)
    return t, x


SETS = [(seed, nrows, overlap, chrom) for seed, (nrows, overlap, chrom) in enumerate(
    [([300, 300], "none", "text"), ([300, 300], "all", "text"), ([300, 257], "half", "text"), ([300, 257], "half", "int"),
     ([200, 1, 333], "half", "text"), ([150, 150, 150], "all", "int"), ([64, 65, 63], "none", "int"),
     ([400, 300, 200, 100], "half", "text"), ([90, 90, 90, 90], "all", "text"), ([120, 80, 1, 256], "half", "int")], start=40)]


@pytest.mark.parametrize("seed,nrows,overlap,chrom", SETS, ids=[f"F{len(s[1])}-{s[2]}-{s[3]}" for s in SETS])
def test_merge_twin_equals_the_host_path(tmp_path, seed, nrows, overlap, chrom):
    paths, chicago, targets = mi.make_set(tmp_path, seed, nrows, overlap, chrom)
    t, x = same_as_host(paths, chicago, targets, tmp_path, (seed, overlap))
    m = t["merged"]
    if overlap == "all":
        assert m["n_out"] == max(nrows) and len(x) > 10                          # keys of two or more files pass the replicate rule
    if overlap == "none":
        assert m["n_out"] == sum(nrows) and len(x) == 0 and len(t["filtered"]) > 5
    if overlap == "half":
        assert max(nrows) < m["n_out"] < sum(nrows)
    assert np.isnan(m["dist"]).any()                                             # trans rows: NA keys match each other
    baits = [set(d["ints"][2].tolist()) for d in t["files"]]
    assert overlap == "all" or all(b - set().union(*(o for o in baits if o is not b)) for b in baits)   # baits that one file alone holds


def test_merge_twin_equals_the_host_path_without_the_replicate_rule(tmp_path):
    paths, chicago, targets = mi.make_set(tmp_path, 77, [500, 400], "half", "text", per_file=1)
    t, x = same_as_host(paths, chicago, targets, tmp_path, "per_file=1")
    assert 50 < len(x) < t["merged"]["n_out"] and len(t["filtered"]) > 2


def word_rows():
    """Rows that differ from the first in ONE of the eight words each (and in what must follow it: a bait's name, a trans row's
    dist), with values whose top bits are set, plus pairs whose two halves of one composite sort word pull in opposite directions."""
    return [mi.base_row(), mi.base_row(baitChr="chr10", oeChr="chr10"), mi.base_row(baitChr="chr2", oeChr="chr2", baitID=3), mi.base_row(baitStart=99),
            mi.base_row(baitStart=2147483647), mi.base_row(baitEnd=2147483647), mi.base_row(baitEnd=-200), mi.base_row(baitID=4, baitName="g4"),
            mi.base_row(baitID=2147483646, baitName="gmax"), mi.base_row(oeChr="chrX", dist="NA"), mi.base_row(oeChr="~~~~~~~~", dist="NA"),
            mi.base_row(oeStart=2147483646), mi.base_row(oeStart=-900), mi.base_row(oeEnd=-5), mi.base_row(oeEnd=2147483647),
            mi.base_row(oeID=2000000000), mi.base_row(oeID=0), mi.base_row(oeEnd=951, oeID=1), mi.base_row(baitEnd=201, baitID=1, baitName="g1"),
            mi.base_row(baitChr="abcdefgh", oeChr="abcdefgh"), mi.base_row(baitChr="~~~~~~~~", oeChr="~~~~~~~~"),
            mi.base_row(baitChr="chr1\x7f", oeChr="chr1")]


def word_files(tmp):
    rows = word_rows()
    a, b = os.path.join(str(tmp), "wa.txt"), os.path.join(str(tmp), "wb.txt")
    mi.write_file(a, ["A0", "B0"], rows[::-1])                                  # against the sorted order: a dropped pass shows
    mi.write_file(b, ["A1", "B1"], rows[3:] + rows[:1])
    chicago, targets, _ = mi.design(2)
    return [a, b], chicago, targets, rows


def test_merge_order_is_the_order_of_the_eight_words(tmp_path):
    paths, chicago, targets, rows = word_files(tmp_path)
    t, x = same_as_host(paths, chicago, targets, tmp_path, "words")
    assert t["merged"]["n_out"] == len(rows) and len(x) == len(rows) - 2 - 2     # (what one file alone holds goes, and the two trans rows)


# ---- decline cases ------------------------------------------------------------------------------------------------------------------------
def decline_cases(tmp):
    """{name: (paths, targets, chicagoData, the twin's reason)}: every case the device hands to the host."""
    chicago, targets, names = mi.design(2)
    good = [mi.base_row(oeID=9 + k, oeStart=900 + k) for k in range(6)]
    out = {}

    def case(name, rows_a, rows_b, why, names_a=names[0], names_b=names[1], targets=targets):
        a, b = os.path.join(str(tmp), f"{name}_a.txt"), os.path.join(str(tmp), f"{name}_b.txt")
        mi.write_file(a, names_a, rows_a)
        mi.write_file(b, names_b, rows_b)
        out[name] = ([a, b], targets, chicago, why)
    case("duplicate_key", good + [good[2]], good, "duplicate key")
    case("bait_name", good, [mi.base_row(oeID=30, baitName="other")] + good[1:], "name disagreement")
    case("oe_name", good, good[:3] + [r[:9] + ["named"] + r[10:] for r in good[3:4]], "name disagreement")
    case("dist", good, [r[:10] + ["801.5"] + r[11:] for r in good[:1]] + good[1:], "dist disagreement")
    case("dist_na", good, [r[:10] + ["NA"] + r[11:] for r in good[:1]] + good[1:], "dist disagreement")
    case("long_chr", [mi.base_row(baitChr="chr1_random", oeChr="chr1_random")] + good, good, "long chromosome name")
    case("ambiguous_chr", [mi.base_row(baitChr="1.0")] + good, good, "ambiguous chromosome token")
    case("na_chr", good, [mi.base_row(oeChr="NA")] + good, "ambiguous chromosome token")
    ints = [mi.base_row(baitChr=7, oeChr=7, oeID=9 + k) for k in range(4)]
    case("int_against_text", ints, good, "integer against text")
    case("header_only", good, [], "no rows")
    case("target_in_two_files", good, good, "target in two files", names_b=["A0", "B1"], targets=["A0", "B0", "B1"])
    return out


CASES = ["duplicate_key", "bait_name", "oe_name", "dist", "dist_na", "long_chr", "ambiguous_chr", "na_chr", "int_against_text", "header_only",
         "target_in_two_files"]


@pytest.mark.parametrize("name", CASES)
def test_decline_cases_are_recognised_and_the_host_gives_what_the_twin_says(tmp_path, name):
    from chicdiff_amd import pipeline
    paths, targets, chicago, why = decline_cases(tmp_path)[name]
    got = mt.decline(paths, targets)
    assert got is not None and got[0] == why, (name, got)
    call = lambda: pipeline.readAndFilterPeakMatrix(paths, targets, chicago, list(chicago), mi.SCORE, outprefix=str(tmp_path / "h"))
    if got[1] == "raise":
        with pytest.raises(ValueError):
            call()
    else:
        x = call()
        assert list(x.columns[:11]) == mi.KEYS and len(x.columns) == 11 + len(targets)


def test_a_target_that_no_file_holds_raises_the_reference_message(tmp_path):
    from chicdiff_amd import pipeline
    paths, targets, chicago, _ = decline_cases(tmp_path)["dist"]
    with pytest.raises(ValueError, match="All specified targetColumns must be present"):
        mt.decline(paths, targets + ["nowhere"])
    with pytest.raises(ValueError, match="All specified targetColumns must be present"):
        pipeline.readAndFilterPeakMatrix(paths, targets + ["nowhere"], chicago, list(chicago), mi.SCORE, outprefix=str(tmp_path / "h"))


# ---- the library (these fail without the feature) ------------------------------------------------------------------------------------------
NEW_EXPORTS = ["chicdiff_hip_peaks_textkeys_dev", "chicdiff_hip_peaks_merge_dev", "chicdiff_hip_peaks_header", "chicdiff_hip_selftest_peaks_textkeys"]


def test_library_exports_the_new_entry_points(lib):
    L = lib.load_library()
    for s in NEW_EXPORTS:
        assert hasattr(L, s), s
        assert s in lib.EXPORTS, s
    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "chicdiff_hip.h")).read()
    for s in NEW_EXPORTS:
        assert f"int {s}(" in header, s
    for name, value in (("CHICDIFF_PEAKS_ST_CHR_LONG", mt.ST_CHR_LONG), ("CHICDIFF_PEAKS_ST_CHR_AMBIGUOUS", mt.ST_CHR_AMBIGUOUS),
                        ("CHICDIFF_PEAKS_ST_MERGE_DUPLICATE", mt.ST_MERGE_DUPLICATE), ("CHICDIFF_PEAKS_ST_MERGE_NAME", mt.ST_MERGE_NAME),
                        ("CHICDIFF_PEAKS_ST_MERGE_DIST", mt.ST_MERGE_DIST), ("CHICDIFF_PEAKS_MERGE_MAX_FILES", mt.MAX_FILES),
                        ("CHICDIFF_PEAKS_KEY_INT", mt.KEY_INT), ("CHICDIFF_PEAKS_KEY_TEXT", mt.KEY_TEXT), ("CHICDIFF_PEAKS_KEY_MIXED", mt.KEY_MIXED)):
        assert re.search(rf"#define {name} {value}\b", header), name
    assert (lib.PEAKS_ST_CHR_LONG, lib.PEAKS_ST_CHR_AMBIGUOUS, lib.PEAKS_ST_MERGE_DUPLICATE, lib.PEAKS_ST_MERGE_NAME, lib.PEAKS_ST_MERGE_DIST) == \
        (mt.ST_CHR_LONG, mt.ST_CHR_AMBIGUOUS, mt.ST_MERGE_DUPLICATE, mt.ST_MERGE_NAME, mt.ST_MERGE_DIST)


def token_file(tmp, name, bait_tokens, oe_tokens, sep="\t", crlf=False):
    rows = [mi.base_row(baitChr=b, oeChr=o, baitName=f"gene{k};{b}", oeName="." if k % 2 else f"n{k}", oeID=9 + k)
            for k, (b, o) in enumerate(zip(bait_tokens, oe_tokens))]
    path = os.path.join(str(tmp), name)
    mi.write_file(path, ["A0", "B0"], rows, sep=sep, crlf=crlf)
    return path


def key_corpus(tmp):
    """Files whose chromosome columns cover every class and status: (path, note)."""
    text = [t for t in TOKENS if mt.classify(t.encode()) == "text" and "\t" not in t]
    ints = [t for t in TOKENS if mt.classify(t.encode()) == "int"]
    short = [t for t in ints if len(t) < 9]
    out = [(token_file(tmp, "text.txt", text, text[::-1]), "text"), (token_file(tmp, "int.txt", ints, ints[::-1]), "int"),
           (token_file(tmp, "mixed.txt", short + text[:5], (short + text[:5])[::-1]), "mixed"),
           (token_file(tmp, "int_text.txt", ints, ["chrX"] * len(ints)), "int and text"),
           (token_file(tmp, "nine.txt", ints + ["X"], ["X"] * (len(ints) + 1)), "nine digits among strings"),
           (token_file(tmp, "comma.txt", text[:9], text[:9], sep=",", crlf=True), "comma, CRLF")]
    for k, t in enumerate(t for t in TOKENS if mt.classify(t.encode()) in ("long", "ambiguous") and t.strip() == t and t):
        out.append((token_file(tmp, f"bad{k}.txt", ["chr1", t, "chr2"], ["chr1", "chr1", t]), repr(t)))
    paths, _, _ = mi.make_set(tmp, 5, [700, 300], "half", "text")
    paths2, _, _ = mi.make_set(tmp, 6, [257], "none", "int")
    return out + [(p, "set") for p in paths + paths2]


def same_keys(got, path, note):
    t = mt.read_file(path, [])
    assert got["status"] == t["key_status"], note
    assert tuple(got["key_class"]) == t["key_class"], note
    assert np.array_equal(np.asarray(got["name_hash"]), np.array(t["name_hash"], dtype=np.int64).reshape(2, -1)), note
    for k in range(2):
        want = t["chr_keys"][k]
        have = [i for i, v in enumerate(want) if v is not None]                  # (a declined token has no key)
        assert np.array_equal(np.asarray(got["chr_keys"])[k][have], np.array([want[i] for i in have], dtype=np.int64)), (note, k)
    return t


def test_library_host_statement_of_the_text_keys_equals_the_twin(tmp_path, lib):
    seen = set()
    for path, note in key_corpus(tmp_path):
        t = same_keys(lib.selftest_peaks_textkeys(path), path, note)
        seen.add((t["key_class"], t["key_status"]))
    assert {c for c, _ in seen} >= {(mt.KEY_TEXT, mt.KEY_TEXT), (mt.KEY_INT, mt.KEY_INT), (mt.KEY_MIXED, mt.KEY_MIXED), (mt.KEY_INT, mt.KEY_TEXT)}
    assert {s for _, s in seen} >= {0, mt.ST_CHR_LONG, mt.ST_CHR_AMBIGUOUS}


def test_library_header_names(tmp_path, lib):
    path = token_file(tmp_path, "h.txt", ["chr1"], ["chr1"], sep=",")
    names, sep = lib.peaks_header(path)
    assert names == mi.KEYS + ["A0", "B0"] and sep == ord(",")
    assert names == mt.header_names(path)
    bad = str(tmp_path / "bad.txt")
    open(bad, "w").write("baitChr\tbaitStart\tx\n1\t2\t3\n")
    with pytest.raises(ValueError, match="the first 11 columns must be"):
        lib.peaks_header(bad)
    with pytest.raises(ValueError, match="cannot open"):
        lib.peaks_header(str(tmp_path / "missing.txt"))
