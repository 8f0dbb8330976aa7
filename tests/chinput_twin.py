"""The rule of f2's text part, restated in plain Python from the comment above chicdiff_hip_chinput_parse_dev in
include/chicdiff_hip.h: body bytes and the three column positions in, the three int32 columns or the offset of the first malformed
line out.  No device, no library: the tests compare both parsers of the library against this."""
import numpy as np

SEPARATORS = (0x09, 0x20, 0x2C)   # tab, blank, comma
INT32_MAX = 2147483647


def _value(field: bytes):
    """An optional single sign, then at least one digit, then digits only; magnitude <= INT32_MAX.  None = malformed."""
    neg = False
    if field[:1] in (b"+", b"-"):
        neg = field[:1] == b"-"
        field = field[1:]
    if not field or any(not (0x30 <= c <= 0x39) for c in field):
        return None
    field = field.lstrip(b"0") or b"0"
    if len(field) > 10:
        return None
    v = int(field)
    if v > INT32_MAX:
        return None
    return -v if neg else v


def _fields(line: bytes, upto: int):
    """The first upto + 1 fields of a line (fewer when the line has fewer): split at every single separator."""
    out, start = [], 0
    for i, c in enumerate(line):
        if c in SEPARATORS:
            out.append(line[start:i])
            start = i + 1
            if len(out) > upto:
                return out
    out.append(line[start:])
    return out


def parse_line(line: bytes, ib: int, io: int, in_: int):
    """(bait, oe, N) of one non-empty line, or None when it is malformed.  Whatever follows field max(ib, io, in) is not looked at."""
    f = _fields(line, max(ib, io, in_))
    vals = []
    for k in (ib, io, in_):
        if k >= len(f):
            return None
        v = _value(f[k])
        if v is None:
            return None
        vals.append(v)
    return tuple(vals)


def parse_body(body: bytes, cols):
    """-> ("rows", bait, oe, N) as int32 arrays in file order, or ("bad", offset) with the body-relative offset of the first
    malformed line's start."""
    ib, io, in_ = cols
    rows = []
    pos, n = 0, len(body)
    while pos < n:
        nl = body.find(b"\n", pos)
        end = n if nl < 0 else nl
        line = body[pos:end]
        if line.endswith(b"\r"):
            line = line[:-1]          # ONE trailing '\r'
        if line:                      # an empty line is skipped
            r = parse_line(line, ib, io, in_)
            if r is None:
                return ("bad", pos)
            rows.append(r)
        pos = end + 1
    a = np.array(rows, dtype=np.int64).reshape(-1, 3)
    return ("rows", a[:, 0].astype(np.int32), a[:, 1].astype(np.int32), a[:, 2].astype(np.int32))


def split_file(data: bytes):
    """The host part of the rule: leading '#' comment lines, then the header line -> (offset of the body, (ib, io, in)).  A header
    that does not name the three columns gives (offset, None)."""
    pos, n = 0, len(data)
    while pos < n and data[pos:pos + 1] == b"#":
        nl = data.find(b"\n", pos)
        pos = n if nl < 0 else nl + 1
    nl = data.find(b"\n", pos)
    end = n if nl < 0 else nl
    header = data[pos:end]
    if header.endswith(b"\r"):
        header = header[:-1]
    names = [f[1:-1] if len(f) >= 2 and f[:1] == b'"' and f[-1:] == b'"' else f for f in _fields(header, len(header))]
    body = min(end + 1, n)
    try:
        return body, (names.index(b"baitID"), names.index(b"otherEndID"), names.index(b"N"))
    except ValueError:
        return body, None
