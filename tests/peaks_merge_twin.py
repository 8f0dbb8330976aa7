"""The .multimerge rule of include/chicdiff_hip.h (above chicdiff_hip_peaks_textkeys_dev; chicdiff.R:218-228, 234-236) in plain Python:
the class and key of a chromosome token, the hash of a name, the eight-word key, the outer join as a dict union ordered by ``sorted``,
and the conditions under which the device declines.  Written from the rule's text; one file's rows come from tests/peaks_twin.py."""
import re

import numpy as np

import peaks_twin as tw

ST_CHR_LONG, ST_CHR_AMBIGUOUS, ST_MERGE_DUPLICATE, ST_MERGE_NAME, ST_MERGE_DIST = 4, 8, 16, 32, 64
KEY_INT, KEY_TEXT, KEY_MIXED = 0, 1, 2
MAX_FILES = 16
NA_SPELLINGS = [b"", b"#N/A", b"#N/A N/A", b"#NA", b"-1.#IND", b"-1.#QNAN", b"-NaN", b"-nan", b"1.#IND", b"1.#QNAN", b"<NA>", b"N/A", b"NA",
                b"NULL", b"NaN", b"None", b"n/a", b"nan", b"null"]
PLAIN_INT = re.compile(rb"(0|[1-9][0-9]{0,8})\Z")
INF = re.compile(rb"[+-]?(inf|infinity)\Z", re.IGNORECASE)
NUMERIC_BYTES = set(b"0123456789+-.eE ")


def classify(tok):
    """'int' | 'text' | 'long' | 'ambiguous' for one chromosome token (bytes)."""
    if PLAIN_INT.match(tok):
        return "int"
    wordy = any(b not in NUMERIC_BYTES for b in tok)
    if len(tok) == 0 or any(b >= 0x80 for b in tok) or not wordy:
        return "ambiguous"
    if len(tok) > 8:
        return "long"
    if tok in NA_SPELLINGS or INF.match(tok):
        return "ambiguous"
    return "text"


def _signed(u):
    return u - (1 << 64) if u >= (1 << 63) else u


def text_key(tok):
    """At most 8 bytes packed big-endian, zero-padded, the top bit flipped, as a signed 64-bit number: its order is byte order."""
    assert len(tok) <= 8
    return _signed(int.from_bytes(tok.ljust(8, b"\0"), "big") ^ (1 << 63))


def fnv1a(b):
    h = 0xcbf29ce484222325
    for c in b:
        h = ((h ^ c) * 0x100000001b3) & ((1 << 64) - 1)
    return _signed(h)


def column_keys(tokens):
    """(class, status bits, keys) of one chromosome column; a key is None where the token has none in the column's form."""
    kinds = [classify(t) for t in tokens]
    status = (ST_CHR_LONG if "long" in kinds else 0) | (ST_CHR_AMBIGUOUS if "ambiguous" in kinds else 0)
    if all(k == "int" for k in kinds):
        return KEY_INT, status, [int(t) for t in tokens]
    if any(k == "int" and len(t) == 9 for k, t in zip(kinds, tokens)):
        status |= ST_CHR_LONG                                       # a 9-digit number in a column of strings has no 8-byte key
    cls = KEY_MIXED if "int" in kinds else KEY_TEXT
    return cls, status, [text_key(t) if k in ("int", "text") and len(t) <= 8 else None for k, t in zip(kinds, tokens)]


def read_file(path, targets):
    """One file by the single-file rule (tests/peaks_twin.py) plus its text keys: dict(ints, dist, scores, line_off, names, text (the
    four text fields as bytes per row), key_class, key_status, chr_keys [2][n], name_hash [2][n])."""
    data = open(path, "rb").read()
    body_off, sep, cols, names = tw.read_header(data, targets)
    body = data[body_off:]
    r = tw.parse_body(body, sep, cols)
    assert r[0] == "rows", r[:2]
    _, ints, dist, scores, line_off = r
    text = []
    for off in line_off:
        e = body.find(b"\n", int(off))
        f = body[int(off):len(body) if e < 0 else e].split(sep, 10)
        text.append((f[0], f[4], f[5], f[9]))
    cb, sb, kb = column_keys([t[0] for t in text])
    co, so, ko = column_keys([t[2] for t in text])
    return dict(path=path, ints=ints, dist=dist, scores=scores, line_off=line_off, names=names, text=text, key_class=(cb, co),
                key_status=sb | so, chr_keys=[kb, ko], name_hash=[[fnv1a(t[1]) for t in text], [fnv1a(t[3]) for t in text]],
                body_off=body_off, sep=sep, n=len(text))


def header_names(path):
    data = open(path, "rb").read()
    p = 0
    while data[p:p + 1] == b"#":
        p = data.find(b"\n", p) + 1
    e = data.find(b"\n", p)
    line = data[p:len(data) if e < 0 else e].rstrip(b"\r")
    sep = b"\t" if b"\t" in line else (b"," if b"," in line else b" ")
    return [n.decode().strip('"') for n in line.split(sep)]


def same_dist(a, b):
    return a == b or (a != a and b != b)                             # NaN equals NaN, +0 equals -0


def merge(files):
    """The outer join of read_file() results with one class per chromosome column: dict(status, n_out, ints (6, n_out) int32, dist,
    scores (sum T_f, n_out), src_file, src_row).  status != 0: the device declines and no table is given."""
    groups, baitnames, status = {}, {}, 0
    for f, d in enumerate(files):
        for r in range(d["n"]):
            iv = [int(v) for v in d["ints"][:, r]]
            bait = (d["chr_keys"][0][r], iv[0], iv[1], iv[2])
            key = bait + (d["chr_keys"][1][r], iv[3], iv[4], iv[5])
            members = groups.setdefault(key, [])
            if any(g == f for g, _ in members):
                status |= ST_MERGE_DUPLICATE
            for g, q in members:
                if files[g]["name_hash"][1][q] != d["name_hash"][1][r]:
                    status |= ST_MERGE_NAME
                if not same_dist(files[g]["dist"][q], d["dist"][r]):
                    status |= ST_MERGE_DIST
            members.append((f, r))
            if baitnames.setdefault(bait, d["name_hash"][0][r]) != d["name_hash"][0][r]:
                status |= ST_MERGE_NAME
    if status:
        return dict(status=status)
    order = sorted(groups)
    n, T = len(order), sum(d["scores"].shape[0] for d in files)
    ints, dist = np.zeros((6, n), dtype=np.int32), np.zeros(n)
    scores = np.full((T, n), np.nan)
    src_file, src_row = np.zeros(n, dtype=np.int32), np.zeros(n, dtype=np.int64)
    t0 = np.concatenate([[0], np.cumsum([d["scores"].shape[0] for d in files])])
    for k, key in enumerate(order):
        f, r = groups[key][0]
        ints[:, k], dist[k], src_file[k], src_row[k] = files[f]["ints"][:, r], files[f]["dist"][r], f, r
        for g, q in groups[key]:
            scores[t0[g]:t0[g + 1], k] = files[g]["scores"][:, q]
    return dict(status=0, n_out=n, ints=ints, dist=dist, scores=scores, src_file=src_file, src_row=src_row)


def decline(paths, targetColumns):
    """None, or (why, what the host reader gives: 'raise' | 'table') where the device path hands the call to the host.  A target that
    no file holds is no decline: both paths raise the reference's message (ValueError here)."""
    targets = list(targetColumns)
    has = [[t for t in targets if t in header_names(p)[11:]] for p in paths]
    if not all(any(t in h for h in has) for t in targets):
        raise ValueError(tw.MISSING)
    if any(sum(t in h for h in has) > 1 for t in targets):
        return "target in two files", "raise"
    if sum(len(h) for h in has) > tw.MAX_SCORES:
        return "score columns", "table"
    files = [read_file(p, h) for p, h in zip(paths, has)]
    if any(d["n"] == 0 for d in files):
        return "no rows", "table"                                    # (pandas 2.3 lets an empty frame's object keys pass the dtype check)
    if any(d["key_status"] & ST_CHR_LONG for d in files):
        return "long chromosome name", "table"
    if any(d["key_status"] for d in files):
        return "ambiguous chromosome token", "table"
    if len({tuple(c == KEY_INT for c in d["key_class"]) for d in files}) > 1:
        return "integer against text", "raise"
    m = merge(files)
    if m["status"] & ST_MERGE_DUPLICATE:
        return "duplicate key", "table"
    if m["status"] & ST_MERGE_NAME:
        return "name disagreement", "table"
    if m["status"]:
        return "dist disagreement", "table"
    return None


def read_and_filter(paths, targetColumns, chicagoData, score):
    """readAndFilterPeakMatrix on several files by this rule (not declined): dict(columns of the kept rows: the 11 keys and the score
    columns file after file; ``filtered``; ``names``; ``merged``: merge()'s table; ``kept``)."""
    targets = list(targetColumns)
    has = [[t for t in targets if t in header_names(p)[11:]] for p in paths]
    files = [read_file(p, h) for p, h in zip(paths, has)]
    m = merge(files)
    assert m["status"] == 0
    names = [c for d in files for c in d["names"]]
    cond = tw.cond_of_cols(names, chicagoData)
    kept, filtered = tw.filter_rows(m["ints"], m["dist"], m["scores"], score, cond, len(targets) > len(chicagoData))
    out = {tw.KEYS[k]: [] for k in tw.TEXT_FIELDS}
    for k in kept:
        t = files[m["src_file"][k]]["text"][m["src_row"][k]]
        for j, c in enumerate(tw.TEXT_FIELDS):
            out[tw.KEYS[c]].append(t[j].decode())
    for k, name in enumerate(("baitStart", "baitEnd", "baitID", "oeStart", "oeEnd", "oeID")):
        out[name] = m["ints"][k][kept]
    out["dist"] = m["dist"][kept]
    for j, name in enumerate(names):
        out[name] = m["scores"][j][kept]
    return dict(columns=out, filtered=filtered, names=names, merged=m, kept=kept, files=files, cond=cond)
