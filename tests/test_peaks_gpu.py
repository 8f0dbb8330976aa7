"""readAndFilterPeakMatrix on the device (HipContext.parse_peaks_text / read_peaks / filter_peaks and the pipeline mirrors) against the
plain-Python twin of the rule in include/chicdiff_hip.h (tests/peaks_twin.py; tests/test_peaks.py holds the twin to the host reader and
the library's host statement to the twin).  Everything is compared exactly: int32 columns equal, fp64 columns as int64 bit patterns,
line offsets, orders, or the offset of the first malformed line.  Shapes come from hip.peaks_caps(): T the tile, W the staged window."""
import os
import re
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import peaks_inputs as pi  # noqa: E402
import peaks_twin as tw  # noqa: E402

gpu = pytest.mark.gpu
T = W = None   # the tile and the staged window: hip.peaks_caps(), set by the ctx fixture once the library is built


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.int64)


@pytest.fixture(scope="module")
def ctx():
    import __graft_entry__ as g
    g.build()
    from chicdiff_amd import hip
    c = hip.HipContext(0)
    global T, W
    caps = hip.peaks_caps()
    T, W = caps["tile_bytes"], caps["window_bytes"]
    assert 130 < T < W
    yield c
    c.close()


def device(ctx, body, sep, cols):
    """The device parser's outcome in the twin's form, and the Peaks object."""
    from chicdiff_amd import hip
    d_text = ctx.torch.from_numpy(np.frombuffer(body, dtype=np.uint8).copy()).to(ctx.device)
    try:
        pk = ctx.parse_peaks_text(d_text, sep.decode(), cols)
    except hip.ChicdiffHipError as e:
        m = re.search(r"malformed peak matrix row at byte offset (\d+) ", str(e))
        assert m and int(m.group(1)) == e.offset, str(e)
        return ("bad", e.offset), None
    if pk.status & hip.PEAKS_ST_QUOTE:
        return ("quote",), pk
    assert pk.status == 0
    return ("rows", pk.ints.cpu().numpy(), pk.dist.cpu().numpy(), pk.scores.cpu().numpy(), pk.line_off.cpu().numpy()), pk


def same(got, want, tag):
    assert got[0] == want[0], (tag, got[:2] if got[0] != "rows" else "rows", want[:2] if want[0] != "rows" else "rows")
    if want[0] == "bad":
        assert got[1] == want[1], tag
    if want[0] != "rows":
        return
    assert got[1].dtype == np.int32 and got[1].shape == want[1].shape and np.array_equal(got[1], want[1]), tag
    assert got[2].shape == want[2].shape and np.array_equal(bits(got[2]), bits(want[2])), tag
    assert got[3].shape == want[3].shape and np.array_equal(bits(got[3]), bits(want[3])), tag
    assert got[4].dtype == np.int64 and np.array_equal(got[4], want[4]), tag


def check(ctx, body, sep, cols, tag):
    want = tw.parse_body(body, sep, cols)
    got, pk = device(ctx, body, sep, cols)
    same(got, want, tag)
    if want[0] == "rows":
        assert pk.maxbait == (int(want[1][2].max()) if want[1].shape[1] else -1), tag
    return want, pk


def file_body(tmp, name, seed, nrows, ntargets=4, **kw):
    """(body, separator, score fields, path, chicagoData, targets) of a generated file."""
    path = os.path.join(str(tmp), name)
    chicago, targets = pi.make_file(path, seed, nrows, ntargets, **kw)
    data = open(path, "rb").read()
    body_off, sep, cols, _ = tw.read_header(data, targets)
    return data[body_off:], sep, cols, path, chicago, targets


def pad_first_line(body, nbytes):
    """`body` grown to nbytes through the ignored last field of its first line."""
    more = nbytes - len(body)
    assert more >= 0
    nl = body.find(b"\n")
    end = nl - 1 if body[nl - 1:nl] == b"\r" else nl
    return body[:end] + b"x" * more + body[end:]


# ---- 1. parse against the twin -------------------------------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("nrows", [0, 1, 2, 63, 64, 65, 255, 256, 257, 4099, 20011])
def test_parse_equals_the_twin_at_every_size(ctx, tmp_path, nrows):
    body, sep, cols, *_ = file_body(tmp_path, "n.txt", 100 + nrows, nrows, 4 if nrows % 2 else 3, na_rate=0.2)
    want, _ = check(ctx, body, sep, cols, nrows)
    assert want[1].shape[1] == nrows


@gpu
def test_parse_bodies_around_one_and_two_tiles_and_other_layouts(ctx, tmp_path):
    body, sep, cols, *_ = file_body(tmp_path, "t.txt", 7, 60)
    assert len(body) < T - 1
    for nbytes in (T - 1, T, T + 1, 2 * T - 1, 2 * T, 2 * T + 1):
        b = pad_first_line(body, nbytes)
        assert len(b) == nbytes
        check(ctx, b, sep, cols, nbytes)
    # the other separators, CRLF with blank lines, no target columns in front of / behind the scores, the last line without '\n'
    for k, kw in enumerate([dict(sep=","), dict(sep=" "), dict(crlf=True, blank_every=3), dict(extra_columns=False),
                            dict(final_newline=False), dict(crlf=True, final_newline=False, extra_columns=False)]):
        body, sep, cols, *_ = file_body(tmp_path, f"v{k}.txt", 20 + k, 300, 5, **kw)
        want, _ = check(ctx, body, sep, cols, kw)
        assert want[1].shape[1] == 300
    check(ctx, b"\n\r\n\n", b"\t", [11], "blank lines only")
    check(ctx, b"", b"\t", [11, 12], "empty body")


@gpu
def test_parse_a_line_start_at_every_position_of_a_tiles_last_130_bytes(ctx, tmp_path):
    body, sep, cols, *_ = file_body(tmp_path, "c.txt", 9, 6, crlf=True)
    first = body.find(b"\n") + 1                                                   # the second row starts here
    for pos in range(T - 130, T):
        b = b"\n" * (pos - first) + body                                          # blank lines in front: that row starts at `pos`
        want, _ = check(ctx, b, sep, cols, pos)
        assert pos in want[4].tolist()


@gpu
def test_parse_a_text_field_longer_than_the_window_and_than_three_tiles(ctx, tmp_path):
    body, sep, cols, *_ = file_body(tmp_path, "l.txt", 11, 40)
    rows = body.split(b"\n")
    for length in (W + 5, 3 * T + 77):
        for at in (0, 17, 39):
            r = list(rows)
            f = r[at].split(b"\t")
            f[4] = b"g" * length                                                  # baitName, ahead of every score field
            r[at] = b"\t".join(f)
            want, _ = check(ctx, b"\n".join(r), sep, cols, (length, at))
            assert want[1].shape[1] == 40


@gpu
@pytest.mark.parametrize("name,fields", pi.malformed_rows(), ids=[n for n, _ in pi.malformed_rows()])
def test_parse_every_malformed_kind_in_the_first_a_middle_and_the_last_tile(ctx, name, fields):
    good = "\t".join(pi.GOOD).encode() + b"\n"
    bad = "\t".join(fields).encode() + b"\n"
    n = 3 * T // len(good) + 2                                                      # a little over three tiles
    for at in (1, n // 2, n - 1):
        lines = [good] * n
        lines[at] = bad
        lines[n - 1] = bad if at != n - 1 else bad.rstrip(b"\n")                  # a later one too: the SMALLEST offset is reported
        body = b"".join(lines)
        want, _ = check(ctx, body, b"\t", [11, 12], (name, at))
        assert want == ("bad", at * len(good)) and (at * len(good)) // T == (0, 1, 3)[(1, n // 2, n - 1).index(at)]


@gpu
def test_parse_a_quote_gives_the_status_bit_and_writes_no_row(ctx, tmp_path):
    from chicdiff_amd import hip
    torch = ctx.torch
    body, sep, cols, *_ = file_body(tmp_path, "q.txt", 13, 900)
    for at in (0, len(body) // 2, len(body) - 2):
        k = body.find(b"gene", at) if body.find(b"gene", at) >= 0 else body.rfind(b"gene")
        b = body[:k] + b'"' + body[k + 1:]
        assert tw.parse_body(b, sep, cols) == ("quote",)
        got, pk = device(ctx, b, sep, cols)
        assert got == ("quote",) and pk.ints is None and pk.status == hip.PEAKS_ST_QUOTE
        # with room for the rows: nothing is written
        d_text = torch.from_numpy(np.frombuffer(b, dtype=np.uint8).copy()).to(ctx.device)
        ints = torch.full((6, 900), -7, dtype=torch.int32, device=ctx.device)
        dist, scores = torch.full((900,), -7.0, dtype=torch.float64, device=ctx.device), torch.full((len(cols), 900), -7.0, dtype=torch.float64, device=ctx.device)
        off = torch.full((900,), -7, dtype=torch.int64, device=ctx.device)
        import ctypes as C
        info = (C.c_int64 * len(hip.PEAKS_INFO))()
        c = np.asarray(cols, dtype=np.int32)
        rc = ctx.lib.chicdiff_hip_peaks_parse_dev(ctx.h, d_text.data_ptr(), len(b), 9, c.ctypes.data_as(C.POINTER(C.c_int32)), len(c), ints.data_ptr(),
                                                  dist.data_ptr(), scores.data_ptr(), off.data_ptr(), 900, info)
        assert rc == 0 and info[1] == hip.PEAKS_ST_QUOTE
        assert bool((ints == -7).all()) and bool((dist == -7).all()) and bool((scores == -7).all()) and bool((off == -7).all())


# ---- 2. decimals ---------------------------------------------------------------------------------------------------------------------
def token_body(tokens, ncol=8):
    """Rows of ncol score columns (fields 11 ..) holding the tokens; the last row is filled up with NA."""
    key = "\t".join(pi.GOOD[:11])
    toks = list(tokens) + ["NA"] * (-len(tokens) % ncol)
    lines = [key + "\t" + "\t".join(toks[i:i + ncol]) for i in range(0, len(toks), ncol)]
    return ("\n".join(lines) + "\n").encode(), list(range(11, 11 + ncol)), toks


@gpu
def test_decimal_tokens_equal_float_bit_for_bit_and_the_writers_domain_is_never_slow(ctx):
    toks = pi.decimal_tokens(np.random.default_rng(5))
    assert len(toks) >= 20000
    wq = [tw.token_wq(t) for t in toks]
    fast = [t for t, (nd, q) in zip(toks, wq) if nd <= 17 and abs(q) <= 22]
    rest = [t for t, (nd, q) in zip(toks, wq) if not (nd <= 17 and abs(q) <= 22)]
    assert len(fast) >= 15000 and len(rest) >= 60 and "9007199254740993e-5" in fast and "1e-320" in rest
    for name, part in (("fast", fast), ("rest", rest)):
        body, cols, filled = token_body(part)
        got, pk = device(ctx, body, b"\t", cols)
        assert got[0] == "rows"
        want = np.array([float("nan") if t == "NA" else float(t) for t in filled]).reshape(-1, len(cols)).T
        assert np.array_equal(bits(got[3]), bits(want)), name                    # every value, signed zeros included
        if name == "fast":
            assert pk.info["nslow"] == 0                                         # NO token of the writers' domain went to the host
        else:
            assert 40 <= pk.info["nslow"] <= len(part)                           # 20 .. 40 digits, huge / tiny exponents: through the patch
    # dist takes the same route
    body = ("\t".join(pi.GOOD[:10]) + "\t12345678901234567890.5\t1\n" + "\t".join(pi.GOOD[:10]) + "\t-40000.5\t2\n").encode()
    got, pk = device(ctx, body, b"\t", [11])
    assert np.array_equal(bits(got[2]), bits([12345678901234567890.5, -40000.5])) and pk.info["nslow"] == 1


@gpu
def test_a_slow_list_overflow_is_a_status_bit_and_the_mirror_falls_back(ctx, tmp_path, capsys):
    from chicdiff_amd import hip, pipeline
    caps = hip.peaks_caps()
    ncol = 64
    nrows = caps["max_slow"] // ncol + 1                                           # 65 600 slow tokens: 64 more than the list holds
    names = [f"s{k}" for k in range(ncol)]
    key = "\t".join(pi.GOOD[:11])
    path = str(tmp_path / "slow.txt")
    with open(path, "w") as f:
        f.write("\t".join(pi.KEYS + names) + "\n")
        for r in range(nrows):
            f.write(key + "\t" + "\t".join("6.%018d7" % (r * ncol + k) for k in range(ncol)) + "\n")
    pk = ctx.read_peaks(path, names)
    assert pk.status == hip.PEAKS_ST_SLOW_OVERFLOW and pk.ints is None and pk.info["nslow"] == nrows * ncol
    chicago = {"A": {n: n for n in names[:32]}, "B": {n: n for n in names[32:]}}
    want = pipeline.readAndFilterPeakMatrix(path, names, chicago, list(chicago), 5.0, outprefix=str(tmp_path / "h"))
    capsys.readouterr()
    pm = pipeline.readAndFilterPeakMatrix(path, names, chicago, list(chicago), 5.0, outprefix=str(tmp_path / "d"), ctx=ctx, device=True)
    assert "slow-token list" in capsys.readouterr().err
    got = pm.to_frame()
    assert len(got) == len(want) == nrows and list(got.columns) == list(want.columns)
    for c in want.columns:
        assert got[c].tolist() == want[c].tolist(), c
    assert np.array_equal(pm["baitID"].cpu().numpy(), want["baitID"].to_numpy(np.int32))


# ---- 3. filter -----------------------------------------------------------------------------------------------------------------------
def check_filter(ctx, path, chicago, targets, tag):
    t = tw.read_and_filter(path, targets, chicago, pi.SCORE)
    pk = ctx.read_peaks(path, targets)
    assert pk.status == 0 and pk.score_names == t["names"] and pk.info["body"] == t["body_off"]
    a = t["all"]
    same(("rows", pk.ints.cpu().numpy(), pk.dist.cpu().numpy(), pk.scores.cpu().numpy(), pk.line_off.cpu().numpy()),
         ("rows", a["ints"], a["dist"], a["scores"], a["line_off"]), tag)
    r = ctx.filter_peaks(pk, pi.SCORE, t["cond"], len(targets) > len(chicago))
    assert np.array_equal(r["kept_idx"].cpu().numpy(), t["kept"]), tag
    assert np.array_equal(r["baitID"].cpu().numpy(), a["ints"][2][t["kept"]]) and np.array_equal(r["oeID"].cpu().numpy(), a["ints"][5][t["kept"]]), tag
    assert r["filtered_baits"].dtype == ctx.torch.int32 and np.array_equal(r["filtered_baits"].cpu().numpy(), t["filtered"]), tag
    return t


@gpu
@pytest.mark.parametrize("k", range(len(pi.CORPUS)))
def test_read_and_filter_equal_the_twin_on_the_corpus(ctx, tmp_path, k):
    path, chicago, targets = pi.corpus_file(tmp_path, k)
    t = check_filter(ctx, path, chicago, targets, k)
    if pi.CORPUS[k][1] >= 64:
        assert 0 < len(t["kept"]) < pi.CORPUS[k][1] and t["filtered"][0] == 3 and t["filtered"][-1] == 900001


def write_rows(path, rows, names=("A1", "B1")):
    with open(path, "w") as f:
        f.write("\t".join(pi.KEYS + list(names)) + "\n")
        for bait, oe, dist, scores in rows:
            f.write("\t".join(["chr1", "1", "2", str(bait), "g", "chr1", "3", "4", str(oe), ".", dist] + list(scores)) + "\n")


@gpu
def test_filter_no_row_kept_and_every_row_kept(ctx, tmp_path):
    chicago, targets = pi.design(2)
    path = str(tmp_path / "f.txt")
    write_rows(path, [(5 + r % 7, 100 + r, "10", ("1.5", "NA")) for r in range(300)])
    t = check_filter(ctx, path, chicago, targets, "none kept")
    assert len(t["kept"]) == 0 and t["filtered"].tolist() == [5, 6, 7, 8, 9, 10, 11]
    write_rows(path, [(5 + r % 7, 100 + r, "10.5", ("7.5", "NA")) for r in range(300)])
    t = check_filter(ctx, path, chicago, targets, "all kept")
    assert len(t["kept"]) == 300 and len(t["filtered"]) == 0


@gpu
def test_filter_at_both_ends_of_the_id_range(tmp_path):
    """Bait IDs 0 and 2^31 - 2 with adjacent other ends: bait + 1 is compared in 64 bits.  The bait table has one 8-byte word per ID up
    to the largest, 16 GiB here, and the context's workspace only grows: this case has a context of its own, closed at its end."""
    import __graft_entry__ as g
    g.build()
    from chicdiff_amd import hip
    c = hip.HipContext(0)
    try:
        chicago, targets = pi.design(2)
        path = str(tmp_path / "f.txt")
        big = 2 ** 31 - 2
        rows = [(0, 1, "4000", ("9", "9")), (0, 2, "8000", ("9", "9")), (big, big + 1, "4000", ("9", "9")), (big, big - 1, "-4000", ("9", "9")),
                (1, 0, "-4000", ("9", "9")), (big - 5, big, "20000", ("9", "9")), (1, 3, "NA", ("9", "9"))]
        write_rows(path, rows)
        t = check_filter(c, path, chicago, targets, "id range")
        assert t["kept"].tolist() == [1, 5] and t["filtered"].tolist() == [big, 1]   # bait + 1 does not wrap; first appearance orders
    finally:
        c.close()


# ---- 4. mirrors ----------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def experiment(tmp_path_factory):
    from pipeline_inputs import make_experiment
    return make_experiment(tmp_path_factory.mktemp("peaks_experiment"), npeaks=2500)


@gpu
def test_mirror_read_and_filter_to_frame_against_the_host_path(ctx, experiment, tmp_path):
    """make_experiment writes its scores with pandas' shortest round-trip digits, up to 17.  The device path is held to float(token)
    bit for bit through the twin; against the host path everything but the scores is held exactly, and a score within
    HOST_READER_ULPS units in the last place: the pandas reader behind the host path is not correctly rounded from 16 digits on
    (tests/test_peaks.py::test_twin_equals_the_host_reader_on_the_corpus has the measurement and the bound).  On one MI355X 120 to
    142 of the 935 kept values per score column differed from the host reader's."""
    from test_peaks import HOST_READER_ULPS
    from chicdiff_amd import pipeline, settings as st
    settings, truth = experiment
    s = st.asChicdiffSettings(settings)
    args = (s["peakfiles"], s["targetColumns"], s["chicagoData"], list(s["chicagoData"]), s["score"])
    want = pipeline.readAndFilterPeakMatrix(*args, outprefix=str(tmp_path / "h"))
    pm = pipeline.readAndFilterPeakMatrix(*args, outprefix=str(tmp_path / "d"), ctx=ctx, device=True)
    got = pm.to_frame()
    assert open(str(tmp_path / "h") + "_filteredBaits.txt", "rb").read() == open(str(tmp_path / "d") + "_filteredBaits.txt", "rb").read()
    assert list(got.columns) == list(want.columns) and len(got) == len(want) == len(truth["peak_bait"]) > 100
    assert np.array_equal(pm["baitID"].cpu().numpy(), truth["peak_bait"]) and np.array_equal(pm["oeID"].cpu().numpy(), truth["peak_oe"])
    names = list(want.columns[11:])
    for c in [c for c in want.columns if c not in names]:
        if c in ("baitChr", "baitName", "oeChr", "oeName"):
            assert got[c].tolist() == want[c].astype(str).tolist(), c
        elif c == "dist":
            assert np.array_equal(bits(got[c].to_numpy()), bits(want[c].to_numpy(np.float64))), c
        else:
            assert np.array_equal(got[c].to_numpy(np.int64), want[c].to_numpy(np.int64)), c
    t = tw.read_and_filter(s["peakfiles"][0], s["targetColumns"], s["chicagoData"], s["score"])
    assert t["names"] == names
    for c in names:
        a, b, f = bits(got[c].to_numpy()), bits(want[c].to_numpy(np.float64)), bits(t["columns"][c])
        print(f"column {c}: {int((a != b).sum())} of {len(a)} values differ from the host reader's, {int((a != f).sum())} from float(token)")
        assert np.array_equal(a, f), c                                            # the device path: float(token)
        nan = np.isnan(got[c].to_numpy())
        assert np.array_equal(nan, want[c].isna().to_numpy()) and (np.abs(a[~nan] - b[~nan]) <= HOST_READER_ULPS).all(), c


@gpu
def test_mirror_region_universe_from_device_peaks(ctx, experiment):
    from chicdiff_amd import pipeline
    settings, truth = experiment
    want = pipeline.getRegionUniverse(settings, ctx)
    got = pipeline.getRegionUniverse(settings, ctx, device_peaks=True)
    assert set(got) == set(want) and want["region_ptr"].numel() > 100
    for k in want:
        a, b = got[k], want[k]
        a, b = (a.cpu().numpy(), b.cpu().numpy()) if hasattr(a, "cpu") else (np.asarray(a), np.asarray(b))
        assert a.dtype == b.dtype and np.array_equal(a, b), k
    import inspect
    assert inspect.signature(pipeline.chicdiffPipeline).parameters["device_peaks"].default is False
    assert inspect.signature(pipeline.readAndFilterPeakMatrix).parameters["device"].default is False


@gpu
@pytest.mark.parametrize("merged", [False, True])
def test_mirror_candidate_interactions_from_device_peaks(ctx, tmp_path, merged):
    import pandas as pd
    from chicdiff_amd import pipeline
    from test_candidate_interactions import SCORE, _golden_case, _golden_table
    g = _golden_table()
    cols = ["baitID", "minOE", "maxOE", "regionID", "log2FoldChange", "weighted_padj", "OEstart", "OEend", "baitstart", "baitend"]
    output = pd.DataFrame({k: np.asarray(g[k]) for k in cols})
    case = _golden_case()
    P = 4000
    names = ["A", "B"] if merged else ["a1", "a2", "b1", "b2"]
    order = names[::-1]                                                            # the file holds the columns in another order
    peaks = pd.DataFrame({"baitChr": 19, "baitStart": 1, "baitEnd": 2, "baitID": case["peak_baitID"][:P], "baitName": [f"gene{i}" for i in range(P)],
                          "oeChr": 19, "oeStart": 3, "oeEnd": 4, "oeID": case["peak_oeID"][:P], "oeName": ".", "dist": 1000})
    for c in order:
        peaks[c] = np.round(case["scores"][names.index(c), :P], 4)   # four decimals: every text reader gives the same double
    path = str(tmp_path / "peaks.txt")
    peaks.to_csv(path, sep="\t", index=False, na_rep="NA")
    chicago = {"A": "a.Rds", "B": "b.Rds"} if merged else {"A": {"a1": "a1.Rds", "a2": "a2.Rds"}, "B": {"b1": "b1.Rds", "b2": "b2.Rds"}}
    settings = dict(chicagoData=chicago, targetColumns=names, score=SCORE, peakfiles=[path])
    mind = 10.0 if merged else 1.0
    want = pipeline.getCandidateInteractions(output, path, settings, minDeltaAsinhScore=mind, ctx=ctx)
    got = pipeline.getCandidateInteractions(output, pipeline.DevicePeakFile(path), settings, minDeltaAsinhScore=mind, ctx=ctx)
    assert len(want) > 5 and len(got) == len(want) and list(got.columns) == list(want.columns)
    for c in want.columns:
        if c == "baitChr":
            assert got[c].tolist() == want[c].astype(str).tolist()
        elif want[c].dtype == np.float64:
            assert np.array_equal(bits(got[c].to_numpy()), bits(want[c].to_numpy())), c
        else:
            assert got[c].tolist() == want[c].tolist(), c


@gpu
def test_mirror_two_peak_files_take_the_host_reader(ctx, tmp_path, capsys):
    from chicdiff_amd import pipeline
    chicago, targets = pi.design(4)
    rows = [(5 + r % 9, 200 + r, "10.5", ("7.5", "6.25")) for r in range(50)]
    f1, f2 = str(tmp_path / "a.txt"), str(tmp_path / "b.txt")
    write_rows(f1, rows, names=("A1", "A2"))
    write_rows(f2, rows[:40], names=("B1", "B2"))                                  # the last ten rows: B1, B2 NA after the outer merge
    args = ([f1, f2], targets, chicago, list(chicago), 5.0)
    want = pipeline.readAndFilterPeakMatrix(*args, outprefix=str(tmp_path / "h"))
    capsys.readouterr()
    pm = pipeline.readAndFilterPeakMatrix(*args, outprefix=str(tmp_path / "d"), ctx=ctx, device=True)
    assert "more than one peak file" in capsys.readouterr().err
    got = pm.to_frame()
    assert len(want) == 40 and len(got) == 40 and list(got.columns) == list(want.columns)
    for c in want.columns:
        assert got[c].tolist() == want[c].tolist(), c
    assert np.array_equal(pm["oeID"].cpu().numpy(), want["oeID"].to_numpy(np.int32))
    assert open(str(tmp_path / "h") + "_filteredBaits.txt", "rb").read() == open(str(tmp_path / "d") + "_filteredBaits.txt", "rb").read()
