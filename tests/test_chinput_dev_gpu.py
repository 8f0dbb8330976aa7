"""f2, text part on the device (HipContext.parse_chinput_text, read_chinput(device=True), getFullRegionData(device_chinput=True))
against the plain-Python twin of the rule in include/chicdiff_hip.h (tests/chinput_twin.py; tests/test_chinput_dev.py holds the host
parser to it): the three int32 columns and the row count exactly, or the offset of the first malformed line.  No tolerance enters.
Shapes come from hip.chinput_caps(): T the tile, L the lane chunk, W the staged window."""
import os
import re
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import chinput_inputs as ci  # noqa: E402
import chinput_twin as tw  # noqa: E402
from test_chinput import write_chinput  # noqa: E402

gpu = pytest.mark.gpu
T, L, W = 16384, 64, 16640   # hip.chinput_caps(), asserted below: the shapes around them are parametrised


@pytest.fixture(scope="module")
def ctx():
    import __graft_entry__ as g
    g.build()
    from chicdiff_amd import hip
    c = hip.HipContext(0)
    caps = hip.chinput_caps()
    assert (caps["tile_bytes"], caps["lane_bytes"], caps["window_bytes"]) == (T, L, W)
    yield c
    c.close()


def device(ctx, body, cols):
    """The device parser's outcome in the twin's form."""
    from chicdiff_amd import hip
    torch = ctx.torch
    d_text = torch.from_numpy(np.frombuffer(body, dtype=np.uint8).copy()).to(ctx.device)
    try:
        out = ctx.parse_chinput_text(d_text, cols)
    except hip.ChicdiffHipError as e:
        m = re.search(r"malformed chinput row at byte offset (\d+) ", str(e))
        assert m and int(m.group(1)) == e.offset, str(e)
        return ("bad", e.offset)
    return ("rows",) + tuple(a.cpu().numpy() for a in out)


def same(got, want, tag):
    assert got[0] == want[0], (tag, got[:2] if got[0] == "bad" else got[0], want[:2] if want[0] == "bad" else want[0])
    if want[0] == "bad":
        assert got[1] == want[1], tag
        return
    for a, b in zip(got[1:], want[1:]):
        assert a.dtype == b.dtype == np.int32 and a.shape == b.shape and np.array_equal(a, b), tag


def check(ctx, body, cols, tag):
    want = tw.parse_body(body, cols)
    same(device(ctx, body, cols), want, tag)
    return want


def pad_first_line(body, nbytes, sep):
    """`body` grown to nbytes by an ignored trailing field on its first line."""
    more = nbytes - len(body)
    assert more >= 1
    nl = body.find(b"\n")
    end = len(body) if nl < 0 else (nl - 1 if body[nl - 1:nl] == b"\r" else nl)
    return body[:end] + sep + b"x" * (more - 1) + body[end:]


# ---- 1. sizes ------------------------------------------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("v", range(len(ci.VARIANTS)))
def test_equal_to_the_twin_at_every_size(ctx, tmp_path, v):
    """No row (an empty body, blank lines only); one row, one wave of rows, one more or fewer; bodies of one byte fewer than, exactly
    and one byte more than a tile, and around two tiles; many tiles.  In every variant of write_chinput."""
    kw = ci.VARIANTS[v]
    rng = np.random.default_rng(100 + v)
    sep = kw.get("sep", "\t").encode()
    cols = ci.file_bytes(tmp_path, *ci.rows(1, rng), **kw)[2]
    same(device(ctx, b"", cols), ("rows",) + (np.empty(0, np.int32),) * 3, "empty")
    for blanks in (b"\n", b"\r\n\n\r\n", b"\n" * (T + 3), b"\r\n" * T + b"\r"):
        assert len(check(ctx, blanks, cols, "blank lines")[1]) == 0
    for n in (1, 63, 64, 65, 20011):
        data, off, cols = ci.file_bytes(tmp_path, *ci.rows(n, rng), rng=rng, **kw)
        want = check(ctx, data[off:], cols, (kw, n))
        assert want[0] == "rows" and len(want[1]) == n
    for nbytes in (T - 1, T, T + 1, 2 * T - 1, 2 * T + 1):
        n = (nbytes - 64) // 34
        data, off, cols = ci.file_bytes(tmp_path, *ci.rows(n, rng), rng=rng, **kw)
        body = pad_first_line(data[off:], nbytes, sep)
        assert len(body) == nbytes
        want = check(ctx, body, cols, (kw, nbytes))
        assert want[0] == "rows" and len(want[1]) == n


# ---- 2. every alignment --------------------------------------------------------------------------------------------------------
@gpu
def test_rows_do_not_depend_on_the_alignment(ctx, tmp_path):
    """One body of about three tiles, CRLF ends and signed values, behind k blank lines: k = 0 .. 2 L + 1, and the k that put a
    '\\r\\n' pair, a sign and a field separator on either side of the first tile boundary.  The rows are the same for every k."""
    rng = np.random.default_rng(21)
    data, off, cols = ci.file_bytes(tmp_path, *ci.rows(3 * T // 30, rng, signed=True), rng=rng, crlf=True)
    body = data[off:]
    want = tw.parse_body(body, cols)
    assert want[0] == "rows" and (want[2] < 0).sum() > 100 and 2.5 * T < len(body) < 3.5 * T
    ks = set(range(2 * L + 2))
    # the '\n' of a "\r\n" pair, the sign of an otherEndID, the separator behind a baitID: the last of each in the first tile, put
    # first in the second tile and last in the first
    for feature in (rb"\r\n", rb"\n\d+\t-", rb"\n\d+\t"):
        i = [m.end() - 1 for m in re.finditer(feature, body[:T])][-1]
        assert i > T - 600
        ks |= {T - i, T - 1 - i}
    for k in sorted(ks):
        shifted = b"\n" * k + body
        if k in (0, 1, L, 2 * L + 1):
            same(tw.parse_body(shifted, cols), want, ("twin", k))
        same(device(ctx, shifted, cols), want, k)


# ---- 3. long lines -------------------------------------------------------------------------------------------------------------
@gpu
def test_long_lines(ctx):
    rows = b"".join(b"%d\t%d\t%d\t77\tNA\n" % (i + 1, 2 * i + 5, i % 9 + 1) for i in range(300))
    # an ignored trailing field of three tiles, in the middle of ordinary rows
    body = rows + b"7\t8\t9\t" + b"z" * (3 * T) + b"\n" + rows
    assert len(check(ctx, body, (0, 1, 2), "trailing field")[1]) == 601
    # the needed columns behind a first field of two windows (read from global memory, not from the staged window)
    body = b"".join(b"y" * (2 * W) + b"\t%d\t-%d\t%d\n" % (i, i + 1, i + 2) for i in range(5))
    assert check(ctx, body, (1, 2, 3), "first field")[2].tolist() == [-1, -2, -3, -4, -5]
    assert check(ctx, b"y" * (2 * W) + b"\t1\t2", (1, 2, 3), "first field, cut short")[0] == "bad"
    # one line without a newline: short, and longer than a window
    assert [a.tolist() for a in check(ctx, b"12 -13 14", (0, 1, 2), "one line")[1:]] == [[12], [-13], [14]]
    assert check(ctx, b"12,13,14," + b"q" * (2 * T), (2, 1, 0), "one long line")[1].tolist() == [14]
    # a row that starts inside the first tile and ends exactly at the window's end: its '\n' the window's last byte, the first byte
    # behind it, or split from its '\r' by the window's end; the value's last digit is the byte in front
    for ending in (b"\n", b"\r\n"):
        for at in (W - 1, W, W + 1):
            head = rows[: (T - 100) // 2]
            head = head[: head.rfind(b"\n") + 1]
            tail = b"\t5\t6\t1234567" + ending
            line = b"w" * (at + 1 - len(head) - len(tail)) + tail
            body = head + line + rows
            assert body[at:at + 1] == b"\n" and len(head) < T
            want = check(ctx, body, (1, 2, 3), ("window end", ending, at))
            assert want[0] == "rows" and 1234567 in want[3].tolist()


# ---- 4. errors -----------------------------------------------------------------------------------------------------------------
BAD_LINES = {"non-digit": b"12\t1x3\t4\t9\tNA", "missing third column": b"12\t13", "empty needed field": b"12\t\t4\t9\tNA",
             "lone sign": b"12\t-\t4\t9\tNA", "2147483648": b"12\t13\t2147483648\t9\tNA", "-2147483648": b"-2147483648\t13\t4\t9\tNA",
             "\\r\\r\\n": b"\r"}


def error_body(places, kind, ending=b"\n"):
    """About four tiles of rows; the line that covers byte `p` is replaced by the malformed line, for every p in places."""
    lines = [b"%d\t%d\t%d\t77\tNA" % (i + 1, 2 * i + 5, i % 9 + 1) for i in range(4 * T // 17)]
    starts = np.cumsum([0] + [len(x) + len(ending) for x in lines])
    bad = BAD_LINES[kind] if (kind != "\\r\\r\\n" or ending == b"\r\n") else b"\r\r"   # with its ending the line reads "\r\r\n"
    for p in places:
        lines[int(np.searchsorted(starts, p, side="right")) - 1] = bad
    return ending.join(lines) + ending


@gpu
@pytest.mark.parametrize("kind", list(BAD_LINES))
def test_malformed_line_is_reported_at_its_offset(ctx, kind):
    for ending in (b"\n", b"\r\n"):
        nbytes = len(error_body([], kind, ending))
        assert nbytes > 3 * T
        for name, p in (("first tile", 40), ("first tile's end", T - 1), ("middle tile", T + T // 2), ("last tile", nbytes - 30)):
            body = error_body([p], kind, ending)
            want = check(ctx, body, (0, 1, 2), (kind, name))
            assert want[0] == "bad" and abs(want[1] - p) < 64, (kind, name, want)


@gpu
def test_smallest_offset_of_several_malformed_lines(ctx):
    """Malformed lines in different tiles (and two in one tile): the smallest line start is reported, whichever workgroup gets there
    first.  The launcher has one launch shape: one workgroup per tile."""
    for places in ([3 * T + 100, T + 500], [2 * T + 7, 2 * T + 3000, 3 * T + 1], [T - 10, T + 10, 40 + 3 * T]):
        body = error_body(places, "non-digit")
        want = check(ctx, body, (0, 1, 2), places)
        assert want[0] == "bad" and abs(want[1] - min(places)) < 64
    assert len(check(ctx, error_body([], "non-digit"), (0, 1, 2), "no malformed line")[1]) == 4 * T // 17


# ---- 5. the corpus of the CPU test ---------------------------------------------------------------------------------------------
@gpu
def test_corpus(ctx, tmp_path):
    cases = [c for c in ci.corpus(tmp_path) if len(c[1]) <= 3 * T][:300]
    outcomes = {"rows": 0, "bad": 0}
    for k, (_, body, cols) in enumerate(cases):
        outcomes[check(ctx, body, cols, k)[0]] += 1
    assert len(cases) > 200 and min(outcomes.values()) > 50, outcomes


# ---- 6. read_chinput(device=True) ----------------------------------------------------------------------------------------------
def read_both(ctx, path, flags):
    torch = ctx.torch
    a = ctx.read_chinput(path, flags, device=False)
    b = ctx.read_chinput(path, flags, device=True)
    assert a[2] == b[2]
    for x, y in zip(a[:2], b[:2]):
        assert x.dtype == y.dtype and x.shape == y.shape and torch.equal(x, y)
    return a


@gpu
def test_read_chinput_device_equals_host(ctx, tmp_path):
    from chicdiff_amd import hip
    torch = ctx.torch
    rng = np.random.default_rng(6)
    bait, oe, N = ci.rows(20011, rng)
    flags = np.zeros(800_001, np.uint8)
    flags[rng.choice(bait, 3000)] = 1
    d_flags = torch.from_numpy(flags).to(ctx.device)
    path = tmp_path / "s.chinput"
    for kw in (dict(), dict(crlf=True), dict(trailing_newline=False)):
        write_chinput(path, bait, oe, N, rng=rng, **kw)
        for fl in (d_flags, None):
            keys, vals, nrows = read_both(ctx, path, fl)
            assert nrows == 20011 and (keys.numel() == 20011 if fl is None else 1000 < keys.numel() < 20011)
    for text in ("#c\nbaitID\totherEndID\tN\n", "baitID\totherEndID\tN"):                      # header only: no rows
        path.write_text(text)
        keys, vals, nrows = read_both(ctx, path, d_flags)
        assert nrows == 0 and keys.numel() == 0 and vals.numel() == 0
    # the same messages as the host path
    header = "#c\nbaitID\totherEndID\tN\n"
    for text in (None, "#c\nbait\totherEndID\tN\n1\t2\t3\n", header + "1\t2\t3\n4\t5\tx\n", header + "1\t2\t3\n" * 3000 + "1\t2\n", ""):
        if text is None:
            p = tmp_path / "missing.chinput"
        else:
            p = path
            path.write_text(text)
        msgs = []
        for dev in (False, True):
            with pytest.raises(hip.ChicdiffHipError) as e:
                ctx.read_chinput(p, d_flags, device=dev)
            msgs.append(str(e.value))
        assert msgs[0] == msgs[1], msgs
        assert text is None or not text.startswith(header) or re.search(r"malformed chinput row at byte offset \d+ ", msgs[0]), msgs
    # the context remembers which read came last: host after device, device after host, and the table call serves that one
    small, big = tmp_path / "small.chinput", tmp_path / "big.chinput"
    write_chinput(small, bait[:500], oe[:500], N[:500])
    write_chinput(big, bait, oe, N)
    want_small, want_big = ctx.read_chinput(small, None), ctx.read_chinput(big, None)
    for first, second in ((True, False), (False, True), (True, True)):
        ctx.read_chinput(big, None, device=first)
        got = ctx.read_chinput(small, None, device=second)
        assert got[2] == 500 and torch.equal(got[0], want_small[0]) and torch.equal(got[1], want_small[1])
        ctx.read_chinput(small, None, device=first)
        got = ctx.read_chinput(big, None, device=second)
        assert got[2] == 20011 and torch.equal(got[0], want_big[0]) and torch.equal(got[1], want_big[1])


@gpu
def test_parse_entry_point_refuses_bad_arguments(ctx):
    """cap too small is an error before anything is written; columns must be distinct."""
    import ctypes as C
    torch = ctx.torch
    body = b"1\t2\t3\n4\t5\t6\n7\t8\t9\n"
    d_text = torch.from_numpy(np.frombuffer(body, dtype=np.uint8).copy()).to(ctx.device)
    out = torch.full((3, 4), -7, dtype=torch.int32, device=ctx.device)
    nrows, bad = C.c_int64(0), C.c_int64(0)
    call = lambda cols, cap: ctx.lib.chicdiff_hip_chinput_parse_dev(ctx.h, d_text.data_ptr(), len(body), *cols, out[0].data_ptr(), out[1].data_ptr(),
                                                                    out[2].data_ptr(), cap, C.byref(nrows), C.byref(bad))
    assert call((0, 1, 2), 2) != 0 and nrows.value == 3 and bool((out == -7).all())
    assert b"3 rows" in ctx.lib.chicdiff_hip_last_error(ctx.h)
    assert call((0, 1, 1), 4) != 0 and call((0, -1, 2), 4) != 0 and bool((out == -7).all())
    assert call((2, 0, 1), 4) == 0 and nrows.value == 3 and bad.value == -1
    assert out.cpu().numpy()[:, :3].tolist() == [[3, 6, 9], [1, 4, 7], [2, 5, 8]] and bool((out[:, 3] == -7).all())


# ---- 7. the pipeline -----------------------------------------------------------------------------------------------------------
@gpu
def test_mirror_device_chinput_same_blocks(ctx, tmp_path):
    import torch
    from chicdiff_amd import pipeline
    from pipeline_inputs import make_experiment, read_chicago_pickle
    settings = make_experiment(tmp_path, npeaks=2500)[0]
    RU = pipeline.getRegionUniverse(settings, ctx)
    RUc = pipeline.getControlRegionUniverse(settings, RU, ctx, rng=np.random.default_rng(11))
    a = pipeline.getFullRegionData(settings, RU, RUc, ctx=ctx, read_chicago=read_chicago_pickle)
    b = pipeline.getFullRegionData(settings, RU, RUc, ctx=ctx, read_chicago=read_chicago_pickle, device_chinput=True)
    ntensors = 0
    for blk_a, blk_b in zip(a[:2], b[:2]):
        assert set(blk_a) == set(blk_b)
        for k, va in blk_a.items():
            if not isinstance(va, torch.Tensor):
                continue
            vb = blk_b[k]
            assert va.dtype == vb.dtype and va.shape == vb.shape, k
            same_bits = torch.equal(va.view(torch.int64), vb.view(torch.int64)) if va.dtype == torch.float64 else torch.equal(va, vb)
            assert same_bits, k
            ntensors += 1
    assert ntensors >= 6 and int(a[0]["fragN"].sum()) > 0
