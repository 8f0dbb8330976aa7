"""Option "sf_log_table": sf_hist_kernel / sf_list_kernel read log k of a count below K from a table the workgroup fills in LDS with the
very function it replaces.  The size factors — or the refusal — must be the same, bit for bit, with the table (1), without (0), and from a
context with "select_all_rounds" = 1: the radix route, whose row_ratio16_kernel keeps computing the logarithm per count (the reference, as
`classic` in tests/test_size_factors_direct.py).

Inputs: n = 1, 255, 4097 rows; S = 2, 8, 16 and 17 (S > 16 takes the radix route whatever the options).  From 255 rows on every column
holds K - 1, K, K + 1, 1 and 2^31 - 1 and values of both halves of the table (asserted); the single row of n = 1 holds those five values
in turn across its columns.  Then one matrix with a zero in every row (no usable row: the same error), one with a negative count, one with
all counts equal (massive ties).
"""
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
K = int(re.search(r"#define CHICDIFF_SF_LOGK (\d+)", open(os.path.join(ROOT, "chicdiff_amd", "csrc", "global_kernels.hip")).read()).group(1))
SPECIAL = [K - 1, K, K + 1, 1, 2 ** 31 - 1]
SHAPES = [(n, S) for n in (1, 255, 4097) for S in (2, 8, 16, 17)]


def draw(n, S):
    rng = np.random.default_rng(1000 * S + n)
    scale = np.exp(rng.normal(0.0, 0.3, S))  # columns of different depth: size factors away from 1
    base = np.where(rng.random((n, 1)) < 0.5, rng.integers(1, K // 2, (n, 1)), rng.integers(K // 2, K, (n, 1)))  # both halves of the table
    base = np.where(rng.random((n, 1)) < 0.05, rng.integers(K, 4 * K, (n, 1)), base)                             # and beyond it
    k = np.maximum(1, rng.poisson(base * scale[None, :])).astype(np.int64)
    if n == 1:
        k[0] = [SPECIAL[j % 5] for j in range(S)]
    else:
        for j in range(S):
            for t, v in enumerate(SPECIAL):
                k[(11 * t + 3 * j) % n, j] = v
            k[200 + j, j] = 5            # lower half (rows the five values above never take: those stay below 93)
            k[230 + j, j] = K // 2 + 5   # upper half
    return k.astype(np.int32)


@pytest.fixture(scope="module")
def ctxs():
    import __graft_entry__ as g
    g.build()
    from chicdiff_amd import hip
    table, plain, radix = hip.HipContext(0), hip.HipContext(0), hip.HipContext(0)
    plain.set_option("sf_log_table", 0)
    radix.set_option("select_all_rounds", 1)
    yield table, plain, radix
    for c in (table, plain, radix):
        c.close()


def outcome(ctx, counts):
    from chicdiff_amd import hip
    try:
        return "ok", ctx.size_factors(ctx.to_device(counts, np.int32))
    except hip.ChicdiffHipError as e:
        return "error", str(e)


def same(a, b):
    return a[0] == b[0] and (np.array_equal(a[1], b[1], equal_nan=True) if a[0] == "ok" else a[1] == b[1])


def test_inputs_hold_what_they_are_meant_to():
    assert K >= 4
    for n, S in SHAPES:
        k = draw(n, S)
        assert k.shape == (n, S) and k.min() >= 1
        if n == 1:
            assert set(k[0].tolist()) == set(SPECIAL[:S])
            continue
        for j in range(S):
            col = set(k[:, j].tolist())
            assert all(v in col for v in SPECIAL), (n, S, j)
            assert any(0 < v < K // 2 for v in col) and any(K // 2 <= v < K for v in col) and any(v > K + 1 for v in col)


@pytest.mark.gpu
@pytest.mark.parametrize("n,S", SHAPES)
def test_table_changes_no_bit_of_the_size_factors(ctxs, n, S):
    table, plain, radix = ctxs
    k = draw(n, S)
    t, p, r = outcome(table, k), outcome(plain, k), outcome(radix, k)
    print(f"{n} x {S}: {t}")
    assert t[0] == "ok" and np.all(np.isfinite(t[1])) and np.all(t[1] > 0), t
    assert same(t, p), (t, p)
    assert same(t, r), (t, r)
    assert same(outcome(table, k), t)  # the histograms were left zero


@pytest.mark.gpu
@pytest.mark.parametrize("S", [2, 8, 16, 17])
def test_special_matrices(ctxs, S):
    table, plain, radix = ctxs
    n = 4097
    zero = draw(n, S)
    zero[np.arange(n), np.arange(n) % S] = 0  # every row holds a zero: no usable row
    neg = draw(n, S)
    neg[n // 2, S - 1] = -3
    neg[7, 0] = -(2 ** 31)  # NA_integer_
    ties = np.full((n, S), K - 1, dtype=np.int32)
    ties2 = np.full((n, S), K + 1, dtype=np.int32)
    for name, k in (("a zero in every row", zero), ("negative counts", neg), ("all counts K - 1", ties), ("all counts K + 1", ties2)):
        t, p, r = outcome(table, k), outcome(plain, k), outcome(radix, k)
        print(f"{name}, {n} x {S}: {t}")
        assert same(t, p), (name, t, p)
        assert same(t, r), (name, t, r)
        if name == "a zero in every row":
            assert t[0] == "error" and "every gene contains at least one zero" in t[1]
        if name.startswith("all counts"):
            assert t[0] == "ok" and np.allclose(t[1], 1.0, rtol=1e-14)
    ok = draw(255, S)  # and the contexts are as good as before
    assert same(outcome(table, ok), outcome(radix, ok))
