"""The rule of the device table writer in plain Python (include/chicdiff_hip.h, above chicdiff_hip_table_text_dev): a table of
ncol >= 2 columns -> its text.  Built on repr(float) and str(int) alone; tests/test_table_text.py holds it against
DataFrame.to_csv(index=False), the GPU tests hold the library against it.

A column is ("int32" | "int64" | "float64", values) or ("dict", codes or None, [bytes, ...])."""
import math

MAX_COLUMNS, MAX_DICT = 64, 4096


def float_cell(v):
    """NaN of any sign and payload: nothing.  inf / -inf.  Otherwise repr(float): the shortest digits that read back as v, positional
    for -4 < decpt <= 16 (always with a fractional part), else d[.ddd]e+XX."""
    v = float(v)
    if math.isnan(v):
        return b""
    return repr(v).encode()


def check_entry(entry, sep):
    for ch in (sep, b'"', b"\r", b"\n"):
        if ch in entry:
            raise ValueError("table_text: a dictionary entry holds the separator, a quote or a line break (it would need quoting)")


def column_cells(col, n, sep=b","):
    kind = col[0]
    if kind in ("int32", "int64"):
        return [str(int(v)).encode() for v in col[1]]
    if kind == "float64":
        return [float_cell(v) for v in col[1]]
    if kind == "dict":
        codes, entries = col[1], col[2]
        if len(entries) > MAX_DICT:
            raise ValueError("table_text: at most %d dictionary entries" % MAX_DICT)
        for e in entries:
            check_entry(e, sep)
        if codes is None:
            return [entries[0]] * n
        return [entries[int(c)] if int(c) >= 0 else b"" for c in codes]
    raise ValueError("table_text: unknown column kind %r" % (kind,))


def table_text(columns, n, sep=","):
    sep = sep.encode() if isinstance(sep, str) else bytes(sep)
    if not 2 <= len(columns) <= MAX_COLUMNS:
        raise ValueError("table_text: 2 .. %d columns" % MAX_COLUMNS)
    cells = [column_cells(c, n, sep) for c in columns]
    return b"".join(sep.join(row) + b"\n" for row in zip(*cells)) if n else b""


def header_line(names, sep=","):
    return (sep.join(names) + "\n").encode()


def to_frame(columns, names):
    """The same table as a pandas frame (dictionary columns as object columns of str / None)."""
    import numpy as np
    import pandas as pd
    data = {}
    n = max((len(c[1]) for c in columns if c[1] is not None), default=0)
    for name, c in zip(names, columns):
        if c[0] == "dict":
            ent = [e.decode() for e in c[2]]
            data[name] = pd.Series([ent[0]] * n if c[1] is None else [ent[int(k)] if int(k) >= 0 else None for k in c[1]], dtype=object)
        else:
            data[name] = pd.Series(np.asarray(c[1], dtype=c[0]))
    return pd.DataFrame(data)
