"""Inputs of the table-text tests (tests/test_table_text.py, tests/test_table_text_gpu.py): the seeded float corpus and small tables.
Everything is a function of fixed seeds; nothing here imports the library."""
import functools
import struct

import numpy as np


def bits(x):
    return struct.unpack("<Q", struct.pack("<d", x))[0]


def from_bits(b):
    return struct.unpack("<d", struct.pack("<Q", b & (2 ** 64 - 1)))[0]


def _neighbours(b):
    """The bit patterns of a positive finite double and of the doubles next to it (no step below +0 or onto inf)."""
    out = [b]
    if b > 0:
        out.append(b - 1)
    if b + 1 < 0x7ff0000000000000:
        out.append(b + 1)
    return out


@functools.lru_cache(maxsize=None)
def corpus_bits():
    """The float corpus as uint64 bit patterns (read-only array)."""
    rng = np.random.default_rng(30)
    b = []
    # the specials: signed zeros, infinities, NaNs with payloads and sign
    b += [0x0, 0x8000000000000000, 0x7ff0000000000000, 0xfff0000000000000, 0x7ff8000000000000, 0xfff8000000000000,
          0x7ff0000000000001, 0xfff0000000000001, 0x7ff8dead0000beef, 0xffffffffffffffff, 0x7fffffffffffffff, 0x7ff4000000000000]
    # every power of two and its two neighbours: the rounding interval below 2^e is half as wide as the one above
    for e in range(-1074, 1024):
        pb = bits(2.0 ** e)
        for v in _neighbours(pb):
            b += [v, v | 1 << 63] if e % 64 == 0 else [v]
    # 10^k and its neighbours (float("1e<k>") is the correctly rounded double)
    for k in range(-323, 309):
        for v in _neighbours(bits(float("1e%d" % k))):
            b.append(v)
        b.append(bits(-float("1e%d" % k)))
    # small integers, 2^53 and around it
    b += [bits(float(i)) for i in range(0, 2001)]
    b += [bits(-float(i)) for i in range(0, 2001, 7)]
    b += [bits(float(2 ** 53 + d)) for d in (-2, -1, 0, 1, 2)]       # (2^53 + 1 is not a double: it reads as 2^53)
    # the switches of the two forms: just below and at 1e16, 1e-4, 1e-5
    for x in (1e16, 1e-4, 1e-5, 1e15, 1e17, 1e-3, 9999999999999998.0, 0.0001, 0.00001, 123456789012345680.0, 1e22, 1e23):
        b += _neighbours(bits(x)) + [bits(-x)]
    # shortest forms of 1 .. 17 digits, in both forms
    digits = "12345678901234567"
    for n in range(1, 18):
        for ex in (-310, -300, -20, -7, -5, -4, -3, -1, 0, 1, 5, 10, 15, 16, 17, 22, 100, 300):
            b.append(bits(float("%s.%se%d" % (digits[0], digits[1:n] or "0", ex))))
            b.append(bits(float("-9.%se%d" % ("9" * (n - 1) or "0", ex))))
    b += [bits(float(s)) for s in ("12345678901234567", "98765432109876543", "1.7976931348623157e308", "2.2250738585072014e-308",
                                   "2.225073858507201e-308", "5e-324", "1e-323", "4.9406564584124654e-324", "0.3", "0.1", "2.5e-5",
                                   "5e-5", "9.5367431640625e-07", "1.2345678901234567", "123456.78901234567", "4.35", "8.41e21")]
    # subnormals
    b += [int(v) for v in rng.integers(1, 1 << 52, size=2000, dtype=np.uint64)]
    b += [(1 << 52) - 1, 1 << 52, (1 << 52) + 1, 0x7fefffffffffffff, 0xffefffffffffffff]
    fixed = np.array(b, dtype=np.uint64)
    random_bits = rng.integers(0, 2 ** 64, size=200_000, dtype=np.uint64, endpoint=False)
    # what Nav, Bav and score look like: ratios of small integers (means of counts), gamma draws
    ratios = rng.integers(0, 400, size=60_000).astype(np.float64) / rng.integers(1, 9, size=60_000).astype(np.float64)
    gammas = np.concatenate([rng.gamma(2.0, 3.0, size=30_000), rng.gamma(0.3, 1e-3, size=5_000), -rng.gamma(2.0, 3.0, size=5_000)])
    out = np.concatenate([fixed, random_bits, ratios.view(np.uint64), gammas.view(np.uint64)])
    out.setflags(write=False)
    return out


def corpus():
    """The corpus as float64 (a view of ``corpus_bits``: the NaN payloads survive)."""
    return corpus_bits().view(np.float64)


def random_bits(n, seed=31):
    return np.random.default_rng(seed).integers(0, 2 ** 64, size=n, dtype=np.uint64, endpoint=False)


# ---- tables: lists of column specifications the twin and the binding both take ---------------------------------------------------
# ("int32" | "int64" | "float64", array) or ("dict", codes array or None, [bytes, ...])
NAMES = [b"control", b"treated", b"", b"x y", b"chr19", b"a-very-long-entry-" * 10 + b"end"]


def wide_floats(n, rng):
    """n doubles whose cells take the full 24 bytes: negative, 17 digits, three exponent digits."""
    out = []
    while len(out) < n:
        m = rng.integers(1 << 52, 1 << 53, size=4 * n, dtype=np.uint64)
        v = -(m.astype(np.float64) * 2.0 ** -1070)
        out += [x for x in v.tolist() if len(repr(x)) == 24]
    return np.array(out[:n])


def mixed_table(n, ncol, seed, every_float_nan=False):
    """ncol columns cycling through the kinds, values from the corpus."""
    rng = np.random.default_rng(seed)
    c = corpus()
    cols = []
    for j in range(ncol):
        kind = j % 5
        if kind == 0:
            cols.append(("int32", rng.integers(-2 ** 31, 2 ** 31, size=n, dtype=np.int64).astype(np.int32)))
        elif kind == 1:
            v = c[rng.integers(0, len(c), size=n)].copy()
            if every_float_nan:
                v[:] = np.nan
            cols.append(("float64", v))
        elif kind == 2:
            cols.append(("dict", rng.integers(-1, len(NAMES), size=n).astype(np.int32), list(NAMES)))
        elif kind == 3:
            v = rng.integers(-2 ** 63, 2 ** 63 - 1, size=n, dtype=np.int64)
            v[: min(n, 4)] = [0, -1, 2 ** 63 - 1, -2 ** 63][: min(n, 4)]
            cols.append(("int64", v))
        else:
            cols.append(("float64", (rng.integers(0, 400, size=n) / rng.integers(1, 9, size=n)).astype(np.float64)))
    return cols


def countput_shaped(n, seed):
    """Two integer ID columns, four float64 columns and one constant ``condition`` column (a null code pointer)."""
    rng = np.random.default_rng(seed)
    score = rng.gamma(2.0, 3.0, size=n)
    score[rng.random(n) < 0.1] = np.nan
    return [("int32", rng.integers(1, 800_000, size=n).astype(np.int32)), ("int32", rng.integers(1, 800_000, size=n).astype(np.int32)),
            ("float64", rng.integers(0, 400, size=n) / rng.integers(1, 5, size=n).astype(np.float64)),
            ("float64", rng.gamma(1.5, 2.0, size=n)), ("float64", score),
            ("float64", rng.integers(1, 10 ** 8, size=n).astype(np.float64) / 2.0), ("dict", None, [b"treated"])]


COUNTPUT_HEADER = ["baitID", "otherEndID", "Nav", "Bav", "score", "oeID_mid", "condition"]
