"""Tables as text on the device (HipContext.table_text / write_table, table_text_kernels.hip) against the plain-Python twin of the rule
above chicdiff_hip_table_text_dev in include/chicdiff_hip.h (tests/table_text_twin.py; tests/test_table_text.py holds the twin to
pandas' to_csv).  Every comparison is of bytes and exact."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import table_text_inputs as ti  # noqa: E402
import table_text_twin as tw  # noqa: E402

gpu = pytest.mark.gpu
ROWS, LDS = 256, 65536   # hip.table_text_caps(), asserted below: the shapes around them are parametrised


@pytest.fixture(scope="module")
def ctx():
    import __graft_entry__ as g
    g.build()
    from chicdiff_amd import hip
    caps = hip.table_text_caps()
    assert (caps["rows_per_tile"], caps["lds_bytes"]) == (ROWS, LDS)
    c = hip.HipContext(0)
    yield c
    c.close()


def upload(ctx, cols):
    """The twin's column specifications as the binding takes them."""
    torch = ctx.torch
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(ctx.device)
    out = []
    for c in cols:
        if c[0] == "dict":
            out.append((None if c[1] is None else dev(c[1]), list(c[2])))
        else:
            out.append(dev(np.asarray(c[1], dtype=c[0])))
    return out


def device_text(ctx, cols, n, sep=","):
    return ctx.table_text(upload(ctx, cols), sep=sep, n=n).cpu().numpy().tobytes()


@pytest.fixture(scope="module")
def corpus_cells():
    return [tw.float_cell(v) for v in ti.corpus().tolist()]


@gpu
def test_float_formatting_on_the_device_equals_the_twin_on_the_whole_corpus(ctx, corpus_cells):
    torch = ctx.torch
    v = ti.corpus()
    assert ctx.selftest_format_double_dev(torch.from_numpy(v.copy()).to(ctx.device)) == corpus_cells
    perm = np.random.default_rng(4).permutation(len(v))                         # another launch, every value on another lane
    got = ctx.selftest_format_double_dev(torch.from_numpy(v[perm]).to(ctx.device))
    back = [None] * len(v)
    for k, p in enumerate(perm.tolist()):
        back[p] = got[k]
    assert back == corpus_cells


SIZES = [0, 1, 63, 64, 65, 255, 256, 257, 511, 513, 20011]
SHAPES = [(n, ncol) for n in SIZES for ncol in (2, 7, 25, 64)]


@gpu
@pytest.mark.parametrize("n,ncol", SHAPES, ids=[f"{n}x{c}" for n, c in SHAPES])
def test_table_text_equals_the_twin_at_every_size(ctx, n, ncol):
    """No row, one row, around a wave, around one and two tiles, many tiles with a last partial one; 2 to 64 columns of every kind
    (dictionary columns with negative codes among them).  Both separators below 1 000 rows; above, they alternate."""
    cols = ti.mixed_table(n, ncol, seed=1000 * ncol + n)
    seps = (",", "\t") if n < 1000 else ((",", "\t")[SHAPES.index((n, ncol)) % 2],)
    d_cols = upload(ctx, cols)
    for sep in seps:
        want = tw.table_text(cols, n, sep)
        got = ctx.table_text(d_cols, sep=sep, n=n).cpu().numpy().tobytes()
        assert len(got) == len(want), (n, ncol, sep)
        assert got == want, (n, ncol, sep)


@gpu
def test_rows_of_the_greatest_width_go_through_the_buffer_in_chunks(ctx):
    """64 columns of 24-byte cells: a tile's text is 256 x 1 600 bytes, more than six LDS buffers; rows straddle the chunk boundaries.
    The same with long dictionary entries between them, and with a last tile of 88 rows."""
    rng = np.random.default_rng(8)
    n = 600
    cols = [("float64", ti.wide_floats(n, rng)) for _ in range(64)]
    want = tw.table_text(cols, n)
    assert len(want) == n * 1600 and ROWS * 1600 > 6 * LDS and LDS % 1600 != 0
    assert device_text(ctx, cols, n) == want
    long_entries = [bytes([97 + k % 26]) * (4096 - k) for k in range(5)]
    cols = cols[:20] + [("dict", rng.integers(-1, 5, size=n).astype(np.int32), long_entries) for _ in range(3)] + cols[20:40]
    assert device_text(ctx, cols, n, "\t") == tw.table_text(cols, n, "\t")


@gpu
def test_a_tile_starts_at_every_residue_modulo_16(ctx):
    """Tile k holds 256 rows of 4 bytes and one byte more: it starts at byte 1 025 k, so the runs' first bytes take every residue
    modulo 16 and the byte head of the store every length 0 .. 15.  A second table moves the residues by its first tile."""
    tiles = 35
    n = tiles * ROWS + 3
    for first in (1, 1234567):
        a = np.ones(n, dtype=np.int32)
        a[::ROWS] = 10
        a[0] = first
        cols = [("int32", a), ("int64", np.ones(n, dtype=np.int64))]
        want = tw.table_text(cols, n)
        starts = np.cumsum([0] + [len(str(int(v))) + 3 for v in a])[::ROWS]
        assert {int(s) % 16 for s in starts} == set(range(16))
        assert device_text(ctx, cols, n) == want


@gpu
def test_empty_cells(ctx):
    n = 1000
    nan = np.full(n, np.nan)
    nan[::3] = -np.nan
    empty = [("float64", nan), ("dict", np.full(n, -1, dtype=np.int32), [b"never"]), ("float64", nan), ("dict", np.full(n, 2, dtype=np.int32), [b"a", b"b", b""])]
    assert device_text(ctx, empty, n) == b",,,\n" * n                          # every cell empty: the separators and the newline remain
    cols = ti.mixed_table(n, 7, seed=5, every_float_nan=True)                 # every float NaN among other columns
    assert device_text(ctx, cols, n, "\t") == tw.table_text(cols, n, "\t")


@gpu
def test_a_null_code_pointer_is_entry_0_for_every_row(ctx):
    n = 3000
    cols = ti.countput_shaped(n, 2)
    assert cols[-1][1] is None
    want = tw.table_text(cols, n)
    assert want.count(b",treated\n") == n
    assert device_text(ctx, cols, n) == want


@gpu
def test_a_capacity_too_small_gives_the_size_and_writes_nothing(ctx):
    from chicdiff_amd import hip
    torch = ctx.torch
    n = 700
    cols = ti.mixed_table(n, 5, seed=9)
    want = tw.table_text(cols, n)
    arr, n_, keep = hip.table_columns(upload(ctx, cols), n=n, device=ctx.device)
    for cap in (0, 1, len(want) - 1):
        buf = torch.full((len(want),), 0xAB, dtype=torch.uint8, device=ctx.device)
        size = C.c_int64(-1)
        ctx._check(ctx.lib.chicdiff_hip_table_text_dev(ctx.h, arr, 5, n, ord(","), buf.data_ptr() if cap else None, cap, C.byref(size)))
        assert size.value == len(want) and bool((buf == 0xAB).all())
    buf = torch.full((len(want) + 64,), 0xAB, dtype=torch.uint8, device=ctx.device)
    ctx._check(ctx.lib.chicdiff_hip_table_text_dev(ctx.h, arr, 5, n, ord(","), buf.data_ptr(), len(want), C.byref(size)))
    assert buf[: len(want)].cpu().numpy().tobytes() == want and bool((buf[len(want):] == 0xAB).all())   # nothing behind the text


@gpu
def test_refusals_through_the_context(ctx):
    from chicdiff_amd import hip
    torch = ctx.torch
    i = torch.zeros(5, dtype=torch.int32, device=ctx.device)
    with pytest.raises(hip.ChicdiffHipError, match="one-column table is not offered"):
        ctx.table_text([i])
    with pytest.raises(hip.ChicdiffHipError, match="holds the separator, a quote or a line break"):
        ctx.table_text([i, (None, ['say "x"'])])
    with pytest.raises(hip.ChicdiffHipError, match="a dictionary code is not below its column's number of entries"):
        ctx.table_text([i, (torch.tensor([0, 1, 2, 1, 0], dtype=torch.int32, device=ctx.device), ["a", "b"])])
    with pytest.raises(ValueError, match="must be on"):
        ctx.table_text([i, torch.zeros(5, dtype=torch.int32)])
    with pytest.raises(ValueError, match="must be contiguous"):
        ctx.table_text([i, torch.zeros(10, dtype=torch.float64, device=ctx.device)[::2]])


@gpu
def test_write_table_equals_the_twin(ctx, tmp_path):
    """An empty table is its header; a later call appends; a text of many pinned halves (the test handle makes a half 4 KiB) arrives
    whole and in order; the default half gives the same file."""
    names = ti.COUNTPUT_HEADER
    path = str(tmp_path / "t.csv")
    n0, n1, n2 = 0, 3000, 777
    t0, t1, t2 = ti.countput_shaped(n0, 1), ti.countput_shaped(n1, 2), ti.countput_shaped(n2, 3)
    head = tw.header_line(names)
    assert ctx.write_table(path, upload(ctx, t0), names, n=n0) == len(head)
    assert open(path, "rb").read() == head
    want1, want2 = tw.table_text(t1, n1), tw.table_text(t2, n2)
    assert len(want1) > 20 * 4096
    try:
        ctx.set_option("table_write_half_kib", 4)
        assert ctx.write_table(path, upload(ctx, t1), names, append=True, n=n1) == len(want1)
        assert open(path, "rb").read() == head + want1
        assert ctx.write_table(path, upload(ctx, t2), names, append=True, n=n2) == len(want2)
        assert open(path, "rb").read() == head + want1 + want2
    finally:
        ctx.set_option("table_write_half_kib", 0)
    assert ctx.write_table(path, upload(ctx, t1), names, n=n1) == len(head) + len(want1)     # an existing file is replaced
    assert open(path, "rb").read() == head + want1
    fresh = str(tmp_path / "appended.csv")
    assert ctx.write_table(fresh, upload(ctx, t2), names, append=True, n=n2, sep=",") == len(want2)   # append creates; no header
    assert open(fresh, "rb").read() == want2


@gpu
def test_an_unwritable_path_is_named_and_leaves_no_file(ctx, tmp_path):
    from chicdiff_amd import hip
    cols = upload(ctx, ti.countput_shaped(100, 1))
    missing = str(tmp_path / "no_such_directory" / "t.csv")
    with pytest.raises(hip.ChicdiffHipError, match="table_write: cannot open .*no_such_directory.*No such file or directory"):
        ctx.write_table(missing, cols, ti.COUNTPUT_HEADER, n=100)
    assert not os.path.exists(missing) and os.listdir(tmp_path) == []
    created = str(tmp_path / "created.csv")                                    # a call that fails after creating the file removes it
    bad = cols[:-1] + [(ctx.torch.full((100,), 7, dtype=ctx.torch.int32, device=ctx.device), ["only"])]
    with pytest.raises(hip.ChicdiffHipError, match="a dictionary code is not below"):
        ctx.write_table(created, bad, ti.COUNTPUT_HEADER, n=100)
    assert not os.path.exists(created)
    kept = str(tmp_path / "kept.csv")                                          # ... and leaves alone a file it did not create
    open(kept, "wb").write(b"mine\n")
    with pytest.raises(hip.ChicdiffHipError, match="a dictionary code is not below"):
        ctx.write_table(kept, bad, ti.COUNTPUT_HEADER, append=True, n=100)
    assert open(kept, "rb").read() == b"mine\n"


@gpu
def test_round_trip_through_read_peaks_keeps_every_bit(ctx, tmp_path):
    """No twin: a peak matrix written by write_table and read back by read_peaks.  Six integer key columns, four text columns from
    dictionaries, dist and three score columns from the corpus values the reader decides on the device (at most 17 digits, decimal
    exponent within +-22; NaN travels as an empty field)."""
    import peaks_inputs as pi
    torch = ctx.torch
    v = ti.corpus()
    keepable = []
    for x in v[:120000:7].tolist() + v[-100000::3].tolist():
        if x != x:
            keepable.append(x)
            continue
        if x in (float("inf"), float("-inf")):
            continue
        r = repr(x).lstrip("-")
        mant, _, ex = r.partition("e")
        whole, _, frac = mant.partition(".")
        q = int(ex or 0) - len(frac.rstrip("0"))
        if abs(q) <= 22 and abs(int(ex or 0)) <= 22:
            keepable.append(x)
    vals = np.array(keepable)
    n = len(vals) // 4
    assert n > 5000 and np.isnan(vals).any()
    rng = np.random.default_rng(12)
    ints = {k: rng.integers(1, 10 ** 6, size=n).astype(np.int32) for k in ("baitStart", "baitEnd", "baitID", "oeStart", "oeEnd", "oeID")}
    chrs = [f"chr{k}".encode() for k in range(1, 20)]
    names = [f"g{k}".encode() for k in range(300)] + [b"."]
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(ctx.device)
    text = lambda entries: (dev(rng.integers(0, len(entries), size=n).astype(np.int32)), entries)
    floats = [vals[k * n:(k + 1) * n] for k in range(4)]
    cols = [text(chrs), dev(ints["baitStart"]), dev(ints["baitEnd"]), dev(ints["baitID"]), text(names),
            text(chrs), dev(ints["oeStart"]), dev(ints["oeEnd"]), dev(ints["oeID"]), text(names)] + [dev(f) for f in floats]
    path = str(tmp_path / "peaks.txt")
    ctx.write_table(path, cols, pi.KEYS + ["s1", "s2", "s3"], sep="\t", n=n)
    pk = ctx.read_peaks(path, ["s1", "s2", "s3"])
    assert pk.status == 0 and pk.n == n
    for k, name in enumerate(("baitStart", "baitEnd", "baitID", "oeStart", "oeEnd", "oeID")):
        assert np.array_equal(pk.ints[k].cpu().numpy(), ints[name]), name
    got = [pk.dist.cpu().numpy()] + [pk.scores[j].cpu().numpy() for j in range(3)]
    for g, f in zip(got, floats):
        nan = np.isnan(f)
        assert np.array_equal(np.isnan(g), nan)
        assert np.array_equal(g.view(np.uint64)[~nan], f.view(np.uint64)[~nan])


# ---- the mirrors -------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def experiment(tmp_path_factory):
    from pipeline_inputs import make_experiment
    return make_experiment(tmp_path_factory.mktemp("table_write"), npeaks=1200, with_chinput=True)[0]


@gpu
def test_mirrors_write_the_same_files(ctx, experiment, tmp_path, capsys):
    """getFullRegionData(device_countput=True, device_write=True) and IHWcorrection(device_write=True): the files to_csv writes, byte
    for byte, and the same returned frames; a frame with a bool column, or with strings that need quoting, takes the host's to_csv
    after one message."""
    import countput_inputs as cpi
    from chicdiff_amd import pipeline
    from pipeline_inputs import quantile_ihw, read_chicago_pickle
    host, devw = dict(experiment, outprefix=str(tmp_path / "host")), dict(experiment, outprefix=str(tmp_path / "dev"))
    RU = pipeline.getRegionUniverse(host, ctx)
    RUc = pipeline.getControlRegionUniverse(host, RU, ctx, rng=np.random.default_rng(11))
    a = pipeline.getFullRegionData(host, RU, RUc, ctx=ctx, read_chicago=read_chicago_pickle, device_countput=True)
    b = pipeline.getFullRegionData(devw, RU, RUc, ctx=ctx, read_chicago=read_chicago_pickle, device_countput=True, device_write=True)
    cpi.assert_same_frame(b[2], a[2], "countput")
    want = open(host["outprefix"] + "_countput.csv", "rb").read()
    assert want == a[2].to_csv(index=False).encode() and len(a[2]) > 1000 and want.count(b",,") > 0     # (NaN cells among them)
    assert open(devw["outprefix"] + "_countput.csv", "rb").read() == want
    with pytest.raises(ValueError, match="needs device_countput=True"):
        pipeline.getFullRegionData(devw, RU, RUc, ctx=ctx, read_chicago=read_chicago_pickle, device_write=True)
    quoted = pipeline.DESeq2Wrap(host, RU, a[0], ctx=ctx)
    ctl = pipeline.DESeq2Wrap(host, RUc, a[1], suffix="Control", theta=quoted.attrs.get("theta"), ctx=ctx)
    # the experiment's restriction map quotes its chromosome names and the mirror's reader keeps the quotes: to_csv doubles them, so
    # the frame as it stands takes the fallback (checked last); without the quotes it is the device's to write
    assert quoted["OEchr"].str.startswith('"').all()
    out = quoted.assign(OEchr=quoted["OEchr"].str.strip('"'), baitchr=quoted["baitchr"].str.strip('"'))
    out.attrs.update(quoted.attrs)
    capsys.readouterr()
    ra = pipeline.IHWcorrection(host, out, a[0], ctl, a[1], ctx=ctx, ihw=quantile_ihw(), rng=np.random.default_rng(3))
    rb = pipeline.IHWcorrection(devw, out, a[0], ctl, a[1], ctx=ctx, ihw=quantile_ihw(), rng=np.random.default_rng(3), device_write=True)
    assert "writing the results table on the host" not in capsys.readouterr().err
    want = open(host["outprefix"] + "_results.csv", "rb").read()
    assert want == ra.to_csv(index=False).encode() and len(ra) > 100 and ra.dtypes.eq(object).any() and ra.dtypes.eq(np.float64).any()
    assert open(devw["outprefix"] + "_results.csv", "rb").read() == want
    assert list(rb.columns) == list(ra.columns) and all(rb[c].equals(ra[c]) for c in ra.columns)
    # a bool column: the fallback, with its message, and the same file
    flagged = out.assign(significant=out["padj"] < 0.05)
    fa = pipeline.IHWcorrection(dict(host, outprefix=str(tmp_path / "hostb")), flagged, a[0], ctl, a[1], ctx=ctx, ihw=quantile_ihw(),
                                rng=np.random.default_rng(3))
    capsys.readouterr()
    pipeline.IHWcorrection(dict(devw, outprefix=str(tmp_path / "devb")), flagged, a[0], ctl, a[1], ctx=ctx, ihw=quantile_ihw(),
                           rng=np.random.default_rng(3), device_write=True)
    err = capsys.readouterr().err
    assert err.count("writing the results table on the host") == 1 and "dtype bool" in err
    assert open(str(tmp_path / "devb") + "_results.csv", "rb").read() == open(str(tmp_path / "hostb") + "_results.csv", "rb").read() == fa.to_csv(index=False).encode()
    # an entry that needs quoting: the same
    qa = pipeline.IHWcorrection(dict(host, outprefix=str(tmp_path / "hostq")), quoted, a[0], ctl, a[1], ctx=ctx, ihw=quantile_ihw(),
                                rng=np.random.default_rng(3))
    capsys.readouterr()
    pipeline.IHWcorrection(dict(devw, outprefix=str(tmp_path / "devq")), quoted, a[0], ctl, a[1], ctx=ctx, ihw=quantile_ihw(),
                           rng=np.random.default_rng(3), device_write=True)
    err = capsys.readouterr().err
    assert err.count("writing the results table on the host") == 1 and "needs quoting" in err
    assert open(str(tmp_path / "devq") + "_results.csv", "rb").read() == open(str(tmp_path / "hostq") + "_results.csv", "rb").read() == qa.to_csv(index=False).encode()
    assert b'"""' in qa.to_csv(index=False).encode()                            # (to_csv doubles the quotes it keeps)


@gpu
def test_frames_the_device_writer_does_not_take(ctx):
    import pandas as pd
    from chicdiff_amd import pipeline
    ok = pd.DataFrame({"a": np.arange(3, dtype=np.int32), "b": [0.5, np.nan, 2.0], "c": ["x", None, "y"]})
    cols, why = pipeline.frame_columns_dev(ok, ctx)
    assert why is None and len(cols) == 3 and cols[2][1] == ["x", "y"] and cols[2][0].cpu().tolist() == [0, -1, 1]
    assert ctx.table_text(cols).cpu().numpy().tobytes() == ok.to_csv(index=False, header=False).encode()
    for frame, reason in ((ok[["b"]], "fewer than two columns"), (ok.assign(d=[True, False, True]), "dtype bool"),
                          (ok.assign(d=pd.array([1, None, 3], dtype="Int64")), "dtype Int64"), (ok.assign(d=["p,q", "r", "s"]), "needs quoting"),
                          (ok.assign(d=np.float32(1.5)), "dtype float32"), (ok.rename(columns={"a": 'a"'}), "needs quoting"),
                          (ok.assign(d=[1, "r", None]), "not strings")):
        cols, why = pipeline.frame_columns_dev(frame, ctx)
        assert cols is None and reason in why, (reason, why)


@gpu
def test_chicdiffPipeline_forwards_both_keywords(ctx, experiment, tmp_path):
    from chicdiff_amd import pipeline
    from pipeline_inputs import quantile_ihw, read_chicago_pickle
    runs = {}
    for name, kw in (("host", {}), ("dev", dict(device_countput=True, device_write=True))):
        st = dict(experiment, outprefix=str(tmp_path / name))
        out = pipeline.chicdiffPipeline(st, ctx=ctx, read_chicago=read_chicago_pickle, ihw=quantile_ihw(), rng=np.random.default_rng(11), **kw)
        runs[name] = (out, open(st["outprefix"] + "_countput.csv", "rb").read(), open(st["outprefix"] + "_results.csv", "rb").read())
    assert runs["dev"][1] == runs["host"][1] and runs["dev"][2] == runs["host"][2] and len(runs["host"][2]) > 10000
    assert runs["dev"][2] == runs["dev"][0].to_csv(index=False).encode()
