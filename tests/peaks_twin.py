"""The peak-matrix rule of include/chicdiff_hip.h (above chicdiff_hip_peaks_parse_dev) in plain Python: header, lines, fields, the
integer and decimal columns, malformed lines, the four filters of readAndFilterPeakMatrix (chicdiff.R:246-270) and the filtered baits
in order of first appearance.  The decimal rule is ``float(token)`` on a token the grammar admits.  Bytes in, numpy out; no pandas."""
import re

import numpy as np

KEYS = ["baitChr", "baitStart", "baitEnd", "baitID", "baitName", "oeChr", "oeStart", "oeEnd", "oeID", "oeName", "dist"]
INT_FIELDS = (1, 2, 3, 6, 7, 8)          # baitStart, baitEnd, baitID, oeStart, oeEnd, oeID
TEXT_FIELDS = (0, 4, 5, 9)
MAX_SCORES = 64
MISSING = "All specified targetColumns must be present in the peak file(s)"
KEYS_MESSAGE = "peak matrix header: the first 11 columns must be " + ", ".join(KEYS)
DECIMAL = re.compile(rb"[+-]?(\d+(\.\d*)?|\.\d+)([eE][+-]?\d+)?\Z")
INTEGER = re.compile(rb"[+-]?\d+\Z")


def read_header(data, targets):
    """(body offset, separator byte, score fields, score names in file order); ValueError with the library's message otherwise."""
    p = 0
    while p < len(data) and data[p:p + 1] == b"#":
        e = data.find(b"\n", p)
        p = len(data) if e < 0 else e + 1
    names, sep, body = [], b" ", p
    if p < len(data):
        e = data.find(b"\n", p)
        e = len(data) if e < 0 else e
        line = data[p:e]
        if line.endswith(b"\r"):
            line = line[:-1]
        sep = b"\t" if b"\t" in line else (b"," if b"," in line else b" ")
        for name in line.split(sep):
            if len(name) >= 2 and name[:1] == b'"' and name[-1:] == b'"':
                name = name[1:-1]
            names.append(name.decode())
        body = min(e + 1, len(data))
    if names[:11] != KEYS:
        raise ValueError(KEYS_MESSAGE)
    targets = list(targets)
    for t, name in enumerate(targets):
        if name in targets[:t]:
            raise ValueError(f"peak matrix: targetColumn {name} is named twice")
        if name in KEYS:
            raise ValueError(f"peak matrix: targetColumn {name} is one of the 11 key columns")
        found = names[11:].count(name)
        if found == 0:
            raise ValueError(MISSING)
        if found > 1:
            raise ValueError(f"peak matrix: targetColumn {name} is named twice")
    if len(targets) > MAX_SCORES:
        raise ValueError(f"peak matrix: {len(targets)} score columns, the device reader takes {MAX_SCORES}")
    cols = [k for k in range(11, len(names)) if names[k] in targets]
    return body, sep, cols, [names[k] for k in cols]


def lines(body):
    """(offset, line) of every non-blank line: a line starts at the body's first byte or after a '\\n'; one trailing '\\r' is dropped."""
    p, n = 0, len(body)
    while p < n:
        e = body.find(b"\n", p)
        e = n if e < 0 else e
        line = body[p:e]
        if line.endswith(b"\r"):
            line = line[:-1]
        if line:
            yield p, line
        p = e + 1


def decimal(tok):
    """NaN for an empty field or NA, float() for a token of the grammar, None = malformed."""
    if tok == b"" or tok == b"NA":
        return float("nan")
    if not DECIMAL.match(tok):
        return None
    return float(tok.decode())


def integer(tok, not_negative):
    if not INTEGER.match(tok):
        return None
    v = int(tok.decode())
    if abs(v) > 2147483647 or (not_negative and v < 0):
        return None
    return v


def parse_line(line, sep, score_cols):
    """(six ints, dist, scores) or None = malformed.  Nothing behind the last needed field is looked at."""
    last = score_cols[-1] if score_cols else 10
    f = line.split(sep, last + 1)          # at most last + 2 pieces: the tail, if any, stays in one piece
    if len(f) < last + 1:
        return None
    ints = []
    for k in INT_FIELDS:
        v = integer(f[k], k in (3, 8))
        if v is None:
            return None
        ints.append(v)
    vals = [decimal(f[k]) for k in [10] + list(score_cols)]
    if any(v is None for v in vals):
        return None
    return ints, vals[0], vals[1:]


def parse_body(body, sep, score_cols):
    """("quote",) | ("bad", offset of the first malformed line) | ("rows", ints (6, n) int32, dist, scores (nscore, n), line_off)."""
    if b'"' in body:
        return ("quote",)
    I, D, S, L = [], [], [], []
    for off, line in lines(body):
        r = parse_line(line, sep, list(score_cols))
        if r is None:
            return ("bad", off)
        I.append(r[0]); D.append(r[1]); S.append(r[2]); L.append(off)
    n = len(I)
    return ("rows", np.array(I, dtype=np.int32).reshape(n, 6).T.copy(), np.array(D, dtype=np.float64),
            np.array(S, dtype=np.float64).reshape(n, len(score_cols)).T.copy(), np.array(L, dtype=np.int64))


def filter_rows(ints, dist, scores, score, cond_of_col, replicate_rule):
    """(kept row indices in file order, baits without a kept row in order of first appearance)."""
    n = ints.shape[1]
    bait, oe = ints[2].astype(np.int64), ints[5].astype(np.int64)
    kept, order, has = [], [], {}
    for r in range(n):
        keep = any(scores[j, r] > score for j in range(scores.shape[0]))
        if keep and replicate_rule:
            for c in range(max(cond_of_col, default=-1) + 1):
                cnt = sum(1 for j in range(scores.shape[0]) if cond_of_col[j] == c and scores[j, r] == scores[j, r])
                keep = keep and cnt >= 2
        keep = keep and dist[r] == dist[r] and oe[r] != bait[r] + 1 and oe[r] != bait[r] - 1
        b = int(bait[r])
        if b not in has:
            has[b] = False
            order.append(b)
        if keep:
            has[b] = True
            kept.append(r)
    return np.array(kept, dtype=np.int64), np.array([b for b in order if not has[b]], dtype=np.int32)


def cond_of_cols(score_names, chicagoData):
    """The condition (0-based, in dict order; -1 = none) whose replicate names hold each score column (chicdiff.R:256)."""
    conds = list(chicagoData)
    out = []
    for name in score_names:
        hit = [k for k, c in enumerate(conds) if name in chicagoData[c]]
        out.append(hit[0] if hit else -1)
    return out


def text_fields(body, sep, line_off, rows):
    """The four text columns of the given rows, cut from the body as strings."""
    out = {KEYS[k]: [] for k in TEXT_FIELDS}
    for r in rows:
        e = body.find(b"\n", int(line_off[r]))
        f = body[int(line_off[r]):len(body) if e < 0 else e].split(sep, 10)
        for k in TEXT_FIELDS:
            out[KEYS[k]].append(f[k].decode())
    return out


def field_digits(body, sep, line_off, rows, fields):
    """(len(fields), len(rows)) significant digits (token_wq) of the decimal tokens in the given fields of the given rows; 0 for NA,
    an empty field or a zero."""
    out = np.zeros((len(fields), len(rows)), dtype=np.int64)
    for i, r in enumerate(rows):
        e = body.find(b"\n", int(line_off[r]))
        f = body[int(line_off[r]):len(body) if e < 0 else e].rstrip(b"\r").split(sep)
        for j, k in enumerate(fields):
            tok = f[k].decode()
            out[j, i] = 0 if tok in ("", "NA") else token_wq(tok)[0]
    return out


def read_and_filter(path, targetColumns, chicagoData, score):
    """readAndFilterPeakMatrix on one file by this rule: dict(columns of the kept rows: the 11 keys and the score columns in file
    order; ``filtered``: the filtered baits; ``names``: the score names).  Raises ValueError on a header or a row the rule refuses."""
    data = open(path, "rb").read()
    body_off, sep, cols, names = read_header(data, targetColumns)
    body = data[body_off:]
    r = parse_body(body, sep, cols)
    if r[0] == "quote":
        raise ValueError("quote")
    if r[0] == "bad":
        e = ValueError(f"malformed peak matrix row at byte offset {r[1] + body_off}")
        e.offset = r[1]
        raise e
    _, ints, dist, scores, line_off = r
    cond = cond_of_cols(names, chicagoData)
    kept, filtered = filter_rows(ints, dist, scores, score, cond, len(targetColumns) > len(chicagoData))
    out = text_fields(body, sep, line_off, kept)
    for k, name in zip(range(6), ("baitStart", "baitEnd", "baitID", "oeStart", "oeEnd", "oeID")):
        out[name] = ints[k][kept]
    out["dist"] = dist[kept]
    for j, name in enumerate(names):
        out[name] = scores[j][kept]
    return dict(columns=out, filtered=filtered, names=names, all=dict(ints=ints, dist=dist, scores=scores, line_off=line_off),
                kept=kept, cond=cond, sep=sep, cols=cols, body_off=body_off, digits=field_digits(body, sep, line_off, kept, [10] + cols))


def token_wq(tok):
    """(significant digits, q) of a decimal token: its digits without leading zeros and up to the last non-zero one are w, and the
    value is w * 10^q.  (0, 0) for a zero."""
    m = re.match(r"[+-]?(\d*)\.?(\d*)(?:[eE]([+-]?\d+))?\Z", tok)
    ip, fp, ex = m.group(1), m.group(2), int(m.group(3) or 0)
    digits = (ip + fp).lstrip("0")
    if not digits:
        return 0, 0
    stripped = digits.rstrip("0")
    return len(stripped), ex - len(fp) + (len(digits) - len(stripped))
