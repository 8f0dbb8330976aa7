"""Inputs of the peak-matrix tests (tests/test_peaks.py, tests/test_peaks_gpu.py): a seeded corpus of tab-separated peak matrices in
Chicago's makePeakMatrix layout, written examples of every kind of malformed line, and the decimal tokens."""
import math
import os

import numpy as np

KEYS = ["baitChr", "baitStart", "baitEnd", "baitID", "baitName", "oeChr", "oeStart", "oeEnd", "oeID", "oeName", "dist"]
SCORE = 5.0


def fmt_score(v, digits):
    """A score as text: NaN -> NA; 0 digits -> an integer token; else `digits` significant digits (17 = round trip)."""
    if v != v:
        return "NA"
    return str(int(round(v))) if digits == 0 else "%.*g" % (digits, v)


def design(T):
    """(chicagoData, targetColumns) with T score columns: two conditions, T // 2 replicates each (T = 2: one column per condition)."""
    if T == 2:
        return {"A": {"A1": "a"}, "B": {"B1": "b"}}, ["A1", "B1"]
    h = T // 2
    a, b = [f"A{k + 1}" for k in range(h)], [f"B{k + 1}" for k in range(T - h)]
    return {"A": {n: n for n in a}, "B": {n: n for n in b}}, a + b


def make_file(path, seed, nrows, T, na_rate=0.15, max_digits=17, extra_columns=True, sep="\t", crlf=False, blank_every=0, final_newline=True):
    """A peak matrix of nrows rows and T target columns (plus, with extra_columns, one column in front of and one behind them that are
    not targets); scores are written with 0 .. max_digits significant digits.  Rows: ~10 % adjacent other ends, ~5 % trans (dist NA), ~12 % below the score threshold; bait 3 has only filtered rows
    and appears first, bait 900001 likewise and appears last; dist holds .5 values.  Returns (chicagoData, targetColumns)."""
    rng = np.random.default_rng(seed)
    chicago, targets = design(T)
    header = KEYS + (["other0"] if extra_columns else []) + targets + (["other1"] if extra_columns else [])
    eol = "\r\n" if crlf else "\n"
    out = [sep.join(header) + eol]
    bait = np.sort(rng.integers(10, 4000, nrows)) if nrows else np.zeros(0, dtype=np.int64)
    rng.shuffle(bait[: nrows // 3])                                               # baits come back after other baits
    for r in range(nrows):
        b = int(bait[r])
        if nrows >= 3 and r == 0:
            b = 3
        if nrows >= 3 and r == nrows - 1:
            b = 900001
        u = rng.random()
        oe = b + int(rng.choice([-1, 1])) if u < 0.10 else b + int(rng.integers(2, 300)) * int(rng.choice([-1, 1]))
        oe = max(oe, 0)
        dist = "NA" if 0.10 <= u < 0.15 else ("%d" % ((oe - b) * 4000) if rng.random() < 0.5 else "%.1f" % ((oe - b) * 4000 + 0.5))
        sc = rng.gamma(2.0, 3.0, T)
        if 0.15 <= u < 0.27 or b in (3, 900001):
            sc = np.minimum(sc, 4.0)
        sc[rng.random(T) < na_rate] = np.nan
        digits = rng.integers(0, max_digits + 1, T)
        chrom = "chr19" if b % 7 else "chrX"
        pos = lambda i: (i % 500000) * 4000                                         # (coordinates stay below 2^31)
        row = [chrom, str(pos(b)), str(pos(b) + 3999), str(b), f"gene{b};x{r}", chrom, str(pos(oe)), str(pos(oe) + 3999), str(oe), ".", dist]
        if extra_columns:
            row.append("%.3f" % rng.random())
        row += [fmt_score(v, int(d)) if rng.random() > 0.02 else "" for v, d in zip(sc, digits)]   # (an empty field now and then)
        if extra_columns:
            row.append("tail")
        if blank_every and r % blank_every == 0:
            out.append(eol)
        out.append(sep.join(row) + (eol if final_newline or r < nrows - 1 else ""))
    with open(path, "w", newline="") as f:
        f.write("".join(out))
    return chicago, targets


# (seed, rows, target columns, NA rate, most significant digits of a score): 0 .. 3 000 rows, both settings of replicate_rule, NA
# rates up to 30 %.  The last two files hold scores with up to 17 digits: pandas' own float conversion is not correctly
# rounded from 16 digits on, so the comparison with the host reader carries a bound there (tests/test_peaks.py).
CORPUS = [(1, 0, 2, 0.1, 15), (2, 1, 4, 0.0, 15), (3, 2, 2, 0.3, 15), (4, 3, 4, 0.3, 15), (5, 64, 6, 0.2, 15), (6, 257, 2, 0.15, 15),
          (7, 1000, 4, 0.3, 15), (8, 3000, 8, 0.1, 15), (9, 3000, 2, 0.25, 15), (10, 777, 5, 0.3, 15), (11, 1000, 4, 0.2, 17),
          (12, 600, 2, 0.1, 17)]


def corpus_file(tmp, k):
    seed, nrows, T, na, digits = CORPUS[k]
    path = os.path.join(str(tmp), f"peaks_{k}.txt")
    chicago, targets = make_file(path, seed, nrows, T, na_rate=na, max_digits=digits)
    return path, chicago, targets


GOOD = ["chr1", "100", "200", "5", "g5", "chr1", "900", "950", "9", ".", "800.5", "6.5", "7.25"]


def malformed_rows():
    """(name, fields) of one row per kind of malformed line, for a file with the two score columns s1, s2 behind the keys."""
    def row(**kw):
        f = list(GOOD)
        for k, v in kw.items():
            f[int(k[1:])] = v
        return f
    return [("too_few_fields", GOOD[:12]), ("keys_only", GOOD[:10]), ("int_empty", row(f1="")), ("int_na", row(f3="NA")),
            ("int_decimal", row(f2="200.0")), ("int_too_large", row(f7="2147483648")), ("int_sign_only", row(f6="-")),
            ("bait_negative", row(f3="-5")), ("oe_negative", row(f8="-1")), ("dist_text", row(f10="far")), ("dist_na_lower", row(f10="na")),
            ("score_nan_word", row(f11="nan")), ("score_inf", row(f12="inf")), ("score_two_points", row(f11="1.2.3")),
            ("score_exponent_empty", row(f12="1e")), ("score_exponent_sign", row(f12="1e+")), ("score_point_only", row(f11=".")),
            ("score_sign_only", row(f11="+")), ("score_blank_inside", row(f12="1 5")), ("score_hex", row(f11="0x10")),
            ("score_na_tail", row(f12="NAN")), ("score_underscore", row(f11="1_0"))]


def decimal_tokens(rng, n=20000):
    """The decimal corpus: (tokens, must_be_fast flags are computed by the twin)."""
    toks = []
    draws = rng.gamma(2.0, 3.0, n)
    places = rng.integers(0, 18, n)
    k = rng.integers(-20, 21, n)
    for v, p, e in zip(draws, places, k):
        toks.append(repr(round(float(v), int(p)) * 10.0 ** int(e)))
    toks += ["5.", ".5", "+.5", "5E3", "1e-05", "-0.0", "0.000", "000123.4500", "9007199254740993", "9007199254740995",
             "9007199254740993e-5", "9007199254740995e-5", "-9007199254740993", "0e0", "-0", "+0.0e-7"]
    # 17-digit neighbours of halfway points between adjacent doubles
    from fractions import Fraction
    for _ in range(1500):
        x = math.ldexp(float(rng.integers(2 ** 52, 2 ** 53)), int(rng.integers(-70, 10)))
        y = np.nextafter(x, np.inf)
        mid = (Fraction(x) + Fraction(float(y))) / 2
        e10 = math.floor(math.log10(x))
        scaled = mid / Fraction(10) ** (e10 - 16)                                 # 17 digits in front of the point
        for d in (math.floor(scaled), math.floor(scaled) + 1):
            toks.append(f"{d}e{e10 - 16}")
    # slow tokens: 20 .. 40 digits, large exponents, subnormal and overflow ranges
    for nd in range(20, 41):
        toks.append("".join(str(int(c)) for c in rng.integers(1, 10, nd)))
        toks.append("0." + "".join(str(int(c)) for c in rng.integers(1, 10, nd)))
    toks += ["1e-320", "1.7976931348623157e308", "2.2250738585072011e-308", "1e400", "-1e400", "1e-400", "4.9e-324", "1e40", "1e-40",
             "12345678901234567890e5", "1" + "0" * 30, "0." + "0" * 30 + "1"]
    return toks
