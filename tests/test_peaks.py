"""readAndFilterPeakMatrix's rule for the device path (include/chicdiff_hip.h, above chicdiff_hip_peaks_parse_dev) without a GPU:
the plain-Python twin (tests/peaks_twin.py) on written examples, the twin against the current host reader
(pipeline.readAndFilterPeakMatrix, pandas) on a seeded corpus, and the library's host statement of the rule
(chicdiff_hip_selftest_peaks) against the twin.  No tolerance enters: values, NaN patterns and orders are compared exactly."""
import os
import re
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import peaks_inputs as pi  # noqa: E402
import peaks_twin as tw  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAN = float("nan")
HOST_READER_ULPS = 64   # the pandas reader against float(token) at 16 - 17 digits: test_twin_equals_the_host_reader_on_the_corpus


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.int64)


def write(tmp, name, header, rows, sep="\t", eol="\n", final=True, prefix=""):
    text = prefix + sep.join(header) + eol + eol.join(sep.join(r) for r in rows) + (eol if final and rows else "")
    path = os.path.join(str(tmp), name)
    with open(path, "wb") as f:
        f.write(text.encode())
    return path


HEADER = pi.KEYS + ["s1", "s2"]


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as g
    g.build()
    from chicdiff_amd import hip
    return hip


# ---- the twin on written examples ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("sep", ["\t", ",", " "])
def test_twin_separators_crlf_blank_lines_and_na(tmp_path, sep):
    rows = [list(pi.GOOD), list(pi.GOOD), list(pi.GOOD), list(pi.GOOD)]
    rows[1][10], rows[1][11], rows[1][12] = "NA", "", "-0.0"
    rows[2][10], rows[2][11], rows[2][12] = "", "NA", "5E3"
    rows[3][10], rows[3][11], rows[3][12] = "-12.5", "+.5", ""                  # the line ends with a separator: an empty last field
    path = write(tmp_path, "a.txt", HEADER, rows, sep=sep, eol="\r\n", prefix="# made by hand\r\n")
    data = open(path, "rb").read()
    head, rest = data.split(b"\r\n", 1)
    data = head + b"\r\n" + rest.replace(b"\r\n", b"\r\n\r\n\n", 2)                # blank lines behind the header and the first row
    body_off, s, cols, names = tw.read_header(data, ["s2", "s1"])
    assert s == sep.encode() and cols == [11, 12] and names == ["s1", "s2"]      # file order, whatever the order of the targets
    kind, ints, dist, scores, line_off = tw.parse_body(data[body_off:], s, cols)
    assert kind == "rows" and ints.shape == (6, 4) and ints[:, 0].tolist() == [100, 200, 5, 900, 950, 9]
    assert np.array_equal(bits(dist), bits([800.5, NAN, NAN, -12.5]))
    assert np.array_equal(bits(scores), bits([[6.5, NAN, NAN, 0.5], [7.25, -0.0, 5000.0, NAN]]))
    assert all(data[body_off + o:body_off + o + 4] == b"chr1" for o in line_off)
    kept, filtered = tw.filter_rows(ints, dist, scores, 5.0, [0, 1], False)
    assert kept.tolist() == [0] and filtered.tolist() == []                       # rows 1 .. 3: dist NA, dist NA, no score above 5


def test_twin_header_rules(tmp_path):
    ok = write(tmp_path, "h.txt", ['"%s"' % k for k in pi.KEYS] + ["x", "s1", "y", "s2"], [])
    assert tw.read_header(open(ok, "rb").read(), ["s1", "s2"])[2:] == ([12, 14], ["s1", "s2"])
    with pytest.raises(ValueError, match=re.escape(tw.MISSING)):
        tw.read_header(open(ok, "rb").read(), ["s1", "s3"])
    with pytest.raises(ValueError, match="s1 is named twice"):
        tw.read_header(open(ok, "rb").read(), ["s1", "s2", "s1"])
    with pytest.raises(ValueError, match="dist is one of the 11 key columns"):
        tw.read_header(open(ok, "rb").read(), ["s1", "dist"])
    twice = write(tmp_path, "t.txt", pi.KEYS + ["s1", "s1"], [])
    with pytest.raises(ValueError, match="s1 is named twice"):
        tw.read_header(open(twice, "rb").read(), ["s1"])
    swapped = write(tmp_path, "w.txt", pi.KEYS[:3] + ["oeID", "baitName"] + pi.KEYS[5:] + ["s1"], [])
    with pytest.raises(ValueError, match="the first 11 columns must be baitChr"):
        tw.read_header(open(swapped, "rb").read(), ["s1"])
    many = [f"c{k}" for k in range(65)]
    with pytest.raises(ValueError, match="65 score columns"):
        tw.read_header(open(write(tmp_path, "m.txt", pi.KEYS + many, []), "rb").read(), many)


@pytest.mark.parametrize("name,fields", pi.malformed_rows(), ids=[n for n, _ in pi.malformed_rows()])
def test_twin_and_library_agree_on_every_kind_of_malformed_line(tmp_path, lib, name, fields):
    rows = [list(pi.GOOD), list(pi.GOOD), fields, list(pi.GOOD), fields]
    path = write(tmp_path, "bad.txt", HEADER, rows)
    data = open(path, "rb").read()
    body_off, sep, cols, _ = tw.read_header(data, ["s1", "s2"])
    want = tw.parse_body(data[body_off:], sep, cols)
    good = len("\t".join(pi.GOOD)) + 1
    assert want == ("bad", 2 * good), name                                         # the FIRST malformed line
    with pytest.raises(ValueError, match=r"malformed peak matrix row at byte offset %d " % (body_off + 2 * good)) as e:
        lib.selftest_peaks(path, ["s1", "s2"])
    assert e.value.offset == 2 * good


def test_nothing_behind_the_last_needed_field_is_looked_at(tmp_path, lib):
    rows = [list(pi.GOOD) + ["not a number", "x" * 50], list(pi.GOOD[:12])]        # the second row lacks s2
    path = write(tmp_path, "tail.txt", HEADER + ["junk", "more"], rows, final=False)
    for targets, nrows in ((["s1"], 2), (["s1", "s2"], None)):
        if nrows is None:
            with pytest.raises(ValueError, match="malformed"):
                lib.selftest_peaks(path, targets)
        else:
            assert lib.selftest_peaks(path, targets)["info"]["nrows"] == nrows


def test_a_quote_in_the_body_is_a_status_bit(tmp_path, lib):
    rows = [list(pi.GOOD), list(pi.GOOD)]
    rows[1][4] = '"g5"'
    path = write(tmp_path, "q.txt", HEADER, rows)
    data = open(path, "rb").read()
    body_off, sep, cols, _ = tw.read_header(data, ["s1", "s2"])
    assert tw.parse_body(data[body_off:], sep, cols) == ("quote",)
    r = lib.selftest_peaks(path, ["s1", "s2"])
    assert r["info"]["status"] == lib.PEAKS_ST_QUOTE and "ints" not in r


# ---- the twin against the current host reader ----------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def corpus(tmp_path_factory):
    tmp = tmp_path_factory.mktemp("peaks_corpus")
    return [pi.corpus_file(tmp, k) for k in range(len(pi.CORPUS))]


@pytest.mark.parametrize("k", range(len(pi.CORPUS)))
def test_twin_equals_the_host_reader_on_the_corpus(corpus, tmp_path, k):
    """The twin is float(token).  The host reader is pandas' python engine, whose float conversion is NOT correctly rounded from 16
    significant digits on.  Measured with pandas 2.3.3 against float(token) on gamma(2, 3) draws (the corpus's scores) written with
    a fixed number of significant digits: at 15 digits 0 of 200 000 tokens differ; at 16 digits 7 078 of 400 000 differ (1.8 %),
    6 904 of them by one unit in the last place and the worst by 52; at 17 digits 109 223 differ (27 %), 105 555 by one unit and
    the worst by 50 — the large ones are values near 0.01, whose tokens have 18 or more decimal places.  So "twin equal to the host
    reader at 0 .. 17 digits" cannot hold as written, and the host reader stays as it is.  What is held: every value whose token has
    at most 15 significant digits equal bit for bit; a value of 16 or 17 digits (cases 10 and 11 only) within HOST_READER_ULPS = 64
    units in the last place of the host reader's — the reference's own error as measured above, rounded up to a power of two —
    while the twin's side is float(token) itself; NaN patterns, kept rows, order, every other column and _filteredBaits.txt equal.
    The count of differing values is printed."""
    from chicdiff_amd import pipeline
    path, chicago, targets = corpus[k]
    nrows = pi.CORPUS[k][1]
    t = tw.read_and_filter(path, targets, chicago, pi.SCORE)
    assert t["all"]["ints"].shape[1] == nrows
    if nrows == 0:
        assert len(t["kept"]) == 0 and len(t["filtered"]) == 0                   # (pandas cannot type the columns of an empty table)
        return
    x = pipeline.readAndFilterPeakMatrix(path, targets, chicago, list(chicago), pi.SCORE, outprefix=str(tmp_path / "host"))
    assert list(x.columns) == pi.KEYS + t["names"]
    if nrows >= 64:
        assert 0 < len(x) < nrows and len(t["filtered"]) >= 2                    # every filter has something to do
    want = open(str(tmp_path / "host") + "_filteredBaits.txt", "rb").read()
    assert "".join(f"{b}\n" for b in t["filtered"]).encode() == want
    if nrows >= 64:
        assert t["filtered"][0] == 3 and t["filtered"][-1] == 900001             # first appearance decides the order
    assert (len(targets) > len(chicago)) == (pi.CORPUS[k][2] > 2)
    for c in [c for c in x.columns if c not in t["names"]] + t["names"]:          # the score columns last
        got = t["columns"][c]
        assert len(got) == len(x), c
        if c in ("baitChr", "baitName", "oeChr", "oeName"):
            assert list(got) == x[c].astype(str).tolist(), c
        elif c == "dist" or c in t["names"]:
            a, b = bits(got), bits(x[c].to_numpy(np.float64))
            long = t["digits"][([pi.KEYS[10]] + t["names"]).index(c)] >= 16         # tokens pandas may round the other way
            print(f"corpus {k} column {c}: {int((a != b).sum())} of {len(a)} values differ from the host reader's, {int(long.sum())} tokens of 16 or 17 digits")
            assert pi.CORPUS[k][4] > 15 or not long.any()
            assert np.array_equal(a[~long], b[~long]), c                          # values, NaN pattern, order
            assert (np.abs(a[long] - b[long]) <= HOST_READER_ULPS).all(), c        # bit patterns of doubles of one sign are ordered
        else:
            assert np.array_equal(np.asarray(got, dtype=np.int64), x[c].to_numpy(np.int64)), c


# ---- the library's host statement against the twin (these fail without the feature) ---------------------------------------------------
@pytest.mark.parametrize("k", range(len(pi.CORPUS)))
def test_library_host_statement_equals_the_twin_on_the_corpus(corpus, lib, k):
    path, chicago, targets = corpus[k]
    t = tw.read_and_filter(path, targets, chicago, pi.SCORE)
    cond_of_target = [next(i for i, c in enumerate(chicago) if name in chicago[c]) for name in targets]
    r = lib.selftest_peaks(path, targets, score=pi.SCORE, cond_of_target=cond_of_target, replicate_rule=len(targets) > len(chicago))
    a = t["all"]
    assert r["info"]["nrows"] == a["ints"].shape[1] and r["info"]["status"] == 0 and r["info"]["body"] == t["body_off"]
    assert r["info"]["sep"] == 9 and [targets[j] for j in r["score_target"]] == t["names"]
    assert r["ints"].dtype == np.int32 and np.array_equal(r["ints"], a["ints"])
    assert np.array_equal(bits(r["dist"]), bits(a["dist"])) and np.array_equal(bits(r["scores"]), bits(a["scores"]))
    assert np.array_equal(r["line_off"], a["line_off"])
    assert np.array_equal(r["kept_idx"], t["kept"]) and np.array_equal(r["filtered"], t["filtered"])
    assert r["info"]["maxbait"] == (int(a["ints"][2].max()) if a["ints"].shape[1] else -1)


def test_library_header_messages(tmp_path, lib):
    ok = write(tmp_path, "h.txt", pi.KEYS + ["x", "s1", "y", "s2"], [list(pi.GOOD[:11]) + ["1", "6", "2", "7"]], sep=",", prefix="#c\n")
    r = lib.selftest_peaks(ok, ["s2", "s1"])
    assert r["info"]["sep"] == ord(",") and r["score_target"].tolist() == [1, 0] and r["scores"].tolist() == [[6.0], [7.0]]
    cases = [(["s1", "s3"], tw.MISSING), (["s1", "s2", "s1"], "peak matrix: targetColumn s1 is named twice"),
             (["s1", "dist"], "peak matrix: targetColumn dist is one of the 11 key columns")]
    for targets, msg in cases:
        with pytest.raises(ValueError) as e:
            lib.selftest_peaks(ok, targets)
        assert str(e.value) == msg
        with pytest.raises(ValueError) as e2:
            tw.read_header(open(ok, "rb").read(), targets)
        assert str(e2.value) == msg
    swapped = write(tmp_path, "w.txt", pi.KEYS[:3] + ["oeID", "baitName"] + pi.KEYS[5:] + ["s1"], [])
    with pytest.raises(ValueError) as e:
        lib.selftest_peaks(swapped, ["s1"])
    assert str(e.value) == tw.KEYS_MESSAGE
    many = [f"c{k}" for k in range(65)]
    with pytest.raises(ValueError, match="65 score columns, the device reader takes 64"):
        lib.selftest_peaks(write(tmp_path, "m.txt", pi.KEYS + many, []), many)
    with pytest.raises(ValueError, match="cannot open"):
        lib.selftest_peaks(str(tmp_path / "none.txt"), ["s1"])


def test_caps_agree_with_the_header(lib):
    hdr = open(os.path.join(ROOT, "include", "chicdiff_hip.h")).read()
    caps = lib.peaks_caps()
    for key, name in (("tile_bytes", "CHICDIFF_CHINPUT_TILE_BYTES"), ("window_bytes", "CHICDIFF_CHINPUT_WINDOW_BYTES"),
                      ("max_scores", "CHICDIFF_PEAKS_MAX_SCORES"), ("max_slow", "CHICDIFF_PEAKS_MAX_SLOW")):
        assert int(re.search(r"#define\s+" + name + r"\s+(\d+)", hdr).group(1)) == caps[key] > 0
    assert caps["max_scores"] == tw.MAX_SCORES == 64
    assert lib.PEAKS_ST_QUOTE == int(re.search(r"#define\s+CHICDIFF_PEAKS_ST_QUOTE\s+(\d+)", hdr).group(1))
    assert lib.PEAKS_ST_SLOW_OVERFLOW == int(re.search(r"#define\s+CHICDIFF_PEAKS_ST_SLOW_OVERFLOW\s+(\d+)", hdr).group(1))
    assert len(lib.PEAKS_INFO) == int(re.search(r"#define\s+CHICDIFF_PEAKS_INFO_WORDS\s+(\d+)", hdr).group(1))
    mk = open(os.path.join(ROOT, "chicdiff_amd", "csrc", "Makefile")).read()
    srcs = re.search(r"^SRCS\s*:=(.*)$", mk, re.M).group(1)
    assert "peaks_kernels.hip" in srcs and "peaks.hip" in srcs
    # the table of powers of five is the generator's output, not a pasted one
    table = os.path.join(ROOT, "chicdiff_amd", "csrc", "pow5_table.h")
    src = open(os.path.join(ROOT, "tools", "make_pow5_table.py")).read()
    assert "pow5_table.h" in src
    vals = re.findall(r"\{0x([0-9a-f]{16})ull, 0x([0-9a-f]{16})ull\}", open(table).read())
    assert [int(h + l, 16) for l, h in vals] == [5 ** k for k in range(40)]


# ---- the device's decimal conversion, compiled for the host ----------------------------------------------------------------------------
def test_decimal_header_on_the_host_equals_float_bit_for_bit(tmp_path):
    """chicdiff_amd/csrc/peaks_decimal.h is host and device code; this is its host half (tests/peaks_decimal_host.cpp, built here with
    the C++ compiler) on the decimal corpus of the GPU test and on 200 000 random tokens of the domain it decides (at most 19 digits,
    |q| <= 39): every decided value is float(token) bit for bit, no token of at most 17 significant digits and |q| <= 22 is left
    undecided, and tokens outside the domain are reported as slow, not guessed."""
    import shutil
    import subprocess
    cxx = shutil.which("g++") or shutil.which("c++") or shutil.which("clang++") or "/opt/rocm/llvm/bin/clang++"
    exe = str(tmp_path / "peaks_decimal_host")
    subprocess.run([cxx, "-O2", "-std=c++17", "-I", os.path.join(ROOT, "chicdiff_amd", "csrc"), os.path.join(ROOT, "tests", "peaks_decimal_host.cpp"),
                    "-o", exe], check=True)
    rng = np.random.default_rng(31)
    toks = pi.decimal_tokens(np.random.default_rng(5))
    for _ in range(200000):
        nd = int(rng.integers(1, 20))
        digits = str(int(rng.integers(1, 10))) + "".join(str(int(c)) for c in rng.integers(0, 10, nd - 1))
        cut = int(rng.integers(0, nd + 1))
        q = int(rng.integers(-39, 40))
        toks.append(("-" if rng.random() < 0.2 else "") + digits[:cut] + "." + digits[cut:] + "e%d" % (q + nd - cut))
    out = subprocess.run([exe], input="\n".join(toks) + "\n", capture_output=True, text=True, check=True).stdout.split("\n")[:-1]
    assert len(out) == len(toks)
    nslow = 0
    for tok, line in zip(toks, out):
        rc, b = line.split()
        nd, q = tw.token_wq(tok)
        if rc == "2":
            assert not (nd <= 19 and abs(q) <= 39), tok                           # the domain the header decides is decided
            nslow += 1
            continue
        assert rc == "0", tok
        assert int(b, 16) == int(bits([float(tok)])[0]) & (2 ** 64 - 1), tok
    assert nslow >= 40
