"""Chicago tables for the countput tests (tests/test_countput.py, tests/test_countput_gpu.py): the columns pipeline._countput reads,
with N, Bmean, score and distSign drawn PER ROW.  The replicates of a condition draw their (baitID, otherEndID) pairs from one universe
(chicago_tables_inputs.table: baits inside and outside the map, other ends within 70 fragments of them, some outside the map), so
most groups hold a row of several replicates.  About 10 % of Bmean, score and distSign are NaN; Bmean spans e^-9 .. e^9 (a Kahan sum
and a plain one differ) with a few +-inf; a few scores are 0.0 or -0.0; the map has a gap."""
import functools

import numpy as np

import chicago_tables_inputs as cti

ID_MIN = cti.ID_MIN
ORDERS = cti.ORDERS
same_bits = cti.same_bits
FLOAT_COLUMNS = ("Nav", "Bav", "score", "oeID_mid")


@functools.lru_cache(maxsize=None)
def the_map(nid):
    """(midsum int64[nid], chr_codes int32[nid], rmap frame): IDs ID_MIN .. ID_MIN + nid - 1 on two chromosomes, 15 IDs from nid // 3 on
    missing (chr code -1, no row in the frame); start + end is odd for about half of the fragments."""
    import pandas as pd
    rng = np.random.default_rng(nid)
    start = 1000 * np.arange(nid, dtype=np.int64) + rng.integers(0, 100, nid)
    end = start + rng.integers(200, 900, nid)
    chr_codes = np.where(np.arange(nid) < nid // 2, 0, 1).astype(np.int32)
    chr_codes[nid // 3: nid // 3 + 15] = -1
    on = chr_codes >= 0
    rmap = pd.DataFrame({"OEchr": np.array(["1", "2"])[chr_codes[on]], "OEstart": start[on], "OEend": end[on],
                         "otherEndID": (ID_MIN + np.arange(nid, dtype=np.int64))[on]})
    midsum = np.where(on, start + end, 0)
    return midsum, chr_codes, rmap


def values(bait, oe, rng, na=0.1):
    """One replicate's frame over the given pairs, values drawn per row."""
    import pandas as pd
    n = len(bait)
    bmean = np.exp(rng.normal(0, 3.0, n))
    bmean[rng.random(n) < 0.01] = np.inf
    bmean[rng.random(n) < 0.01] = -np.inf
    bmean[rng.random(n) < na] = np.nan
    score = rng.gamma(2.0, 2.0, n) - 1.0
    score[rng.random(n) < 0.03] = 0.0
    score[rng.random(n) < 0.03] = -0.0
    score[rng.random(n) < na] = np.nan
    ds = np.rint(rng.normal(0, 1e5, n))
    ds[rng.random(n) < na] = np.nan
    return pd.DataFrame({"baitID": np.asarray(bait, dtype=np.int32), "otherEndID": np.asarray(oe, dtype=np.int32),
                         "N": rng.integers(1, 400, n).astype(np.int32), "Bmean": bmean, "score": score, "distSign": ds})


def split(total, nrep):
    """``nrep`` different lengths that add up to ``total`` (a length may be 0 when total < nrep (nrep + 1) / 2)."""
    w = np.arange(1, nrep + 1)
    lens = (total * w) // w.sum()
    lens[-1] += total - lens.sum()
    return [int(v) for v in lens]


@functools.lru_cache(maxsize=None)
def condition(lengths, seed=1, order="shuffled", dups=False):
    """The replicates of one condition, ``lengths[r]`` rows each, every replicate in row order ``order``.  Without ``dups`` a pair
    occurs at most once per replicate; with ``dups`` a tenth of a replicate's rows repeat a pair of that replicate.
    Returns (frames, nid)."""
    rng = np.random.default_rng(seed + 7919 * sum(lengths) + len(lengths))
    nmax = max(max(lengths), 1)
    uni = cti.table(nmax + nmax // 4 + 8, seed, False, "keyed")
    ub, uo = uni["baitID"].to_numpy(), uni["otherEndID"].to_numpy()
    nid = cti.nid_of(len(ub))
    ub = np.where(ub == ub.max(), ID_MIN + nid + 50, ub)   # one bait (at least) lies outside the map; its other ends stay where they are
    frames = []
    for r, n in enumerate(lengths):
        at = rng.choice(len(ub), n, replace=False)
        if dups and n > 1:
            k = rng.choice(n, max(1, n // 10), replace=False)
            at[k] = at[rng.integers(0, n, len(k))]
        frames.append(cti.reorder(values(ub[at], uo[at], rng), order, seed + r))
    return frames, nid


def edge_rows(nid):
    """Three replicates whose groups are written out by hand, on baits OUTSIDE the map (they must stay) and other ends on it.
    Returns (frames, expected): expected[k] = (Nav, Bav, score) of group k, groups in order of first appearance."""
    import pandas as pd
    nan, inf = np.nan, np.inf
    oe0 = ID_MIN + 5
    assert the_map(nid)[1][5:5 + 12].min() >= 0
    # group: rows as (replicate, N, Bmean, score)
    groups = [
        [(0, 1, inf, 0.0), (1, 2, 1.0, -0.0), (2, 3, 2.0, nan)],          # [inf, 1, 2] -> inf (NaN without the reset); 0.0 stays
        [(0, 4, 1.0, -0.0), (1, 5, -inf, 0.0)],                           # -inf; -0.0 stays
        [(0, 6, inf, nan), (2, 7, -inf, nan)],                            # inf - inf -> NaN; no score -> NaN
        [(1, 8, nan, -inf), (2, 9, nan, nan)],                            # no Bmean -> NaN; -inf is a value
        [(0, 10, 1.0, 3.0), (1, 11, 2.0 ** -53, 3.0), (2, 12, 2.0 ** -53, 2.0)],   # Kahan: (1 + 2^-52) / 3, plain: 1 / 3
        [(2, 13, 0.25, -inf), (2, 14, 0.5, inf), (2, 15, 0.75, 1.0)],       # a pair repeated inside one replicate
    ]
    rows = [[], [], []]
    for k, grp in enumerate(groups):
        for r, N, b, s in grp:
            rows[r].append((ID_MIN + nid + 100 + k, oe0 + k, N, b, s, 1.0))
    frames = [pd.DataFrame({"baitID": np.array([t[0] for t in rr], dtype=np.int32), "otherEndID": np.array([t[1] for t in rr], dtype=np.int32),
                            "N": np.array([t[2] for t in rr], dtype=np.int32), "Bmean": np.array([t[3] for t in rr], dtype=np.float64),
                            "score": np.array([t[4] for t in rr], dtype=np.float64), "distSign": np.array([t[5] for t in rr], dtype=np.float64)})
              for rr in rows]
    expected = [(2.0, inf, 0.0), (4.5, -inf, -0.0), (6.5, nan, nan), (8.5, nan, -inf), (11.0, (1.0 + 2.0 ** -52) / 3.0, 3.0), (14.0, 0.5, inf)]
    return frames, expected


def with_edges(frames, nid):
    """``frames`` (three replicates) with edge_rows' rows put in front of replicates 0 and 1 and behind replicate 2."""
    import pandas as pd
    e, expected = edge_rows(nid)
    out = [pd.concat([e[0], frames[0]], ignore_index=True), pd.concat([e[1], frames[1]], ignore_index=True),
           pd.concat([frames[2], e[2]], ignore_index=True)]
    return out, expected


REP_BAIT, REP_OE = ID_MIN + 3400, ID_MIN + 40      # a bait outside every map used here, an other end on them


@functools.lru_cache(maxsize=None)
def repeated_pair(scattered, n=20011, reps=5000, seed=9):
    """One replicate of ``n`` rows plus ``reps`` rows of the pair (REP_BAIT, REP_OE) — next to one another from row 7 000 on, or
    scattered across the table — and a second replicate of 65 rows, two of them that pair again.  Returns (frames, nid)."""
    import pandas as pd
    rng = np.random.default_rng(seed)
    (base, small), nid = condition((n, 65), seed)
    tied = values(np.full(reps, REP_BAIT), np.full(reps, REP_OE), rng)
    if not scattered:
        big = pd.concat([base.iloc[:7000], tied, base.iloc[7000:]], ignore_index=True)
    else:
        pos = np.sort(rng.choice(n + reps, reps, replace=False))
        slot = np.empty(n + reps, dtype=np.int64)
        slot[np.setdiff1d(np.arange(n + reps), pos)] = np.arange(n)
        slot[pos] = n + np.arange(reps)
        big = pd.concat([base, tied], ignore_index=True).iloc[slot].reset_index(drop=True)
    small = small.copy()
    small.loc[[3, 60], "baitID"], small.loc[[3, 60], "otherEndID"] = REP_BAIT, REP_OE
    return (big, small), nid


def frame_of(twins, names):
    """The twin's dictionaries, one per condition, as pipeline._countput's frame."""
    import pandas as pd
    out = []
    for t, name in zip(twins, names):
        z = pd.DataFrame({"baitID": t["baitID"], "otherEndID": t["otherEndID"], "Nav": t["Nav"], "Bav": t["Bav"],
                          "score": t["score"], "oeID_mid": t["oeID_mid"]})
        z["condition"] = name
        out.append(z)
    return pd.concat(out, ignore_index=True)


def assert_same_frame(got, want, tag=""):
    assert list(got.columns) == list(want.columns), (tag, list(got.columns), list(want.columns))
    assert len(got) == len(want), (tag, len(got), len(want))
    for k in got.columns:
        assert got[k].dtype == want[k].dtype, (tag, k, got[k].dtype, want[k].dtype)
        if k in FLOAT_COLUMNS:
            assert same_bits(got[k].to_numpy(), want[k].to_numpy()), (tag, k)
        else:
            assert np.array_equal(got[k].to_numpy(), want[k].to_numpy()), (tag, k)
