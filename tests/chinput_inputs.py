"""Inputs of the chinput text tests (tests/test_chinput_dev.py, tests/test_chinput_dev_gpu.py): files in the variants of
tests/test_chinput.py's write_chinput, and the seeded corpus of mutated bodies both tests walk."""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from chinput_twin import split_file  # noqa: E402
from test_chinput import write_chinput  # noqa: E402

# write_chinput's variants: the seven of tests/test_chinput.py (the default, blank separator, CRLF, no trailing newline, no comment line,
# blank lines every 97 rows, header columns permuted) and the comma separator
VARIANTS = [dict(), dict(sep=" "), dict(crlf=True), dict(trailing_newline=False), dict(comment=False), dict(blank_every=97),
            dict(header=("otherEndID", "N", "distSign", "baitID", "otherEndLen")), dict(sep=",")]
ALPHABET = b"0123456789\t, +-\r\nNA"
CORPUS_SEED, CASES_PER_VARIANT = 2100, 36


def rows(n, rng, signed=False):
    bait = np.sort(rng.integers(1, 800_000, n)).astype(np.int32)
    oe = rng.integers(1, 840_000, n).astype(np.int32)
    N = rng.geometric(0.3, n).astype(np.int32)
    if signed:
        oe = np.where(rng.random(n) < 0.3, -oe, oe).astype(np.int32)
    return bait, oe, N


def file_bytes(tmp_dir, bait, oe, N, **kw):
    """The bytes write_chinput writes for these rows -> (whole file, offset of the body, (ib, io, in))."""
    path = os.path.join(str(tmp_dir), "w.chinput")
    write_chinput(path, bait, oe, N, **kw)
    with open(path, "rb") as f:
        data = f.read()
    off, cols = split_file(data)
    return data, off, cols


def corpus(tmp_dir):
    """[(header bytes, body bytes, cols)]: bodies of 400 to 1750 rows in every variant, 0 to 3 bytes of each replaced by draws from
    ALPHABET (the number of replaced bytes drawn with weights 0.1, 0.15, 0.25, 0.5: most replacements
    land in a digit or in a column that is not read, and a quarter of the cases has to fail)."""
    rng = np.random.default_rng(CORPUS_SEED)
    out = []
    for kw in VARIANTS:
        for _ in range(CASES_PER_VARIANT):
            n = int(rng.integers(400, 1750))
            data, off, cols = file_bytes(tmp_dir, *rows(n, rng), rng=rng, **kw)
            body = bytearray(data[off:])
            for _ in range(int(rng.choice(4, p=[0.1, 0.15, 0.25, 0.5]))):
                body[int(rng.integers(0, len(body)))] = ALPHABET[int(rng.integers(0, len(ALPHABET)))]
            out.append((data[:off], bytes(body), cols))
    return out
