"""Adversarial Chicago tables for the background-table tests (tests/test_chicago_tables.py, tests/test_chicago_tables_gpu.py):
the columns pipeline.background_tables reads, with s_j, s_i, Tmean, tblb and tlb drawn PER ROW — not functions of the fragment, as
in pipeline_inputs.make_experiment — so that which row wins a group shows in the result.  About 10 % of the values are NaN and of
the codes NA, some IDs lie outside [ID_MIN, ID_MIN + nid), refBinMean is a function of distbin (an NA distbin has a value of its own)."""
import functools

import numpy as np

ID_MIN = 100
LEVB = ["(0,25]", "(25,60]", "(60,150]"]
LEVL = ["(0,3]", "(3,9]", "(9,30]", "(30,100]"]
NBIN = 12
REFMEAN = np.exp(3.0 - 0.9 * np.log(np.arange(1, NBIN + 1)))
REF_NA_BIN = 0.004                    # refBinMean of the rows without a distbin
ORDERS = ("keyed", "reversed", "shuffled")


def nid_of(n):
    return 400 if n < 4000 else 3000


def _frame(bait, oe, rng, na=0.1):
    import pandas as pd
    n = len(bait)
    val = lambda: np.where(rng.random(n) < na, np.nan, np.exp(rng.normal(0, 0.5, n)))
    lab = lambda lev: np.array(lev + [None], dtype=object)[np.where(rng.random(n) < na, len(lev), rng.integers(0, len(lev), n))]
    k = np.where(rng.random(n) < na, -1, rng.integers(0, NBIN, n))
    ref = np.where(k >= 0, REFMEAN[np.maximum(k, 0)], REF_NA_BIN)
    ref[rng.random(n) < na] = np.nan
    if n:
        k[0], ref[0] = 0, REFMEAN[0]  # the distance function needs one point at least
    return pd.DataFrame({"baitID": np.asarray(bait, dtype=np.int32), "otherEndID": np.asarray(oe, dtype=np.int32), "s_j": val(), "s_i": val(),
                         "tblb": lab(LEVB), "tlb": lab(LEVL), "Tmean": val(),
                         "distbin": np.array([f"bin{b:03d}" if b >= 0 else None for b in k], dtype=object), "refBinMean": ref})


def reorder(x, order, seed=0):
    if order == "keyed":
        return x.sort_values(["baitID", "otherEndID"], kind="stable").reset_index(drop=True)
    if order == "reversed":
        return reorder(x, "keyed").iloc[::-1].reset_index(drop=True)
    assert order == "shuffled"
    return x.sample(frac=1.0, random_state=seed).reset_index(drop=True)


@functools.lru_cache(maxsize=None)
def table(n, seed=1, dups=False, order="shuffled"):
    """n rows over about n / 60 baits, every bait with other ends within 70 fragments of it.  Without ``dups`` every (baitID,
    otherEndID) pair occurs once, so the tables of the three ``order``s hold the same groups with the same winners; with ``dups`` a
    tenth of the rows repeat another row's pair with values of their own, and the winner is the repeat that comes first."""
    rng = np.random.default_rng(seed + 1000 * n)
    nid = nid_of(n)
    nb = max(1, -(-n // 60))
    baits = rng.choice(np.arange(ID_MIN - 5, ID_MIN + nid + 5), nb, replace=False)
    cand = (np.repeat(baits, 141).astype(np.int64) << 32) | (np.repeat(baits, 141) + np.tile(np.arange(-70, 71), nb)).astype(np.int64)
    key = rng.choice(cand, n, replace=False)
    if dups and n > 1:
        at = rng.choice(n, max(1, n // 10), replace=False)
        key[at] = key[rng.integers(0, n, len(at))]
    return reorder(_frame(key >> 32, key & 0xFFFFFFFF, rng), order, seed)


@functools.lru_cache(maxsize=None)
def contention(n=20000, seed=5):
    """Every row on one bait, one window of 50 other ends and one (tblb, tlb) pair: each slot is contended from every workgroup."""
    rng = np.random.default_rng(seed)
    x = _frame(np.full(n, ID_MIN + 200), ID_MIN + 230 + rng.integers(0, 50, n), rng)
    x["tblb"], x["tlb"] = LEVB[1], LEVL[2]
    return x


TIE_BAIT, TIE_OE, TIE_BAIT2 = ID_MIN + 3100, ID_MIN + 3180, ID_MIN + 3120   # outside table()'s baits (nid 3000 + 5) and their windows


@functools.lru_cache(maxsize=None)
def ties(scattered, n=4097, seed=3, reps=200):
    """table(n) plus ``reps`` rows of the pair (TIE_BAIT, TIE_OE) with different values — next to one another (inside a wave's run)
    or scattered across the table — plus one row (TIE_BAIT2, TIE_OE): the same other end under a larger bait.  The tied rows are
    all of TIE_BAIT's, and no smaller bait shows TIE_OE: both fragments' winners are the FIRST tied row in row order.
    Returns (table, index of that row); nid = 3200."""
    import pandas as pd
    rng = np.random.default_rng(seed)
    base = table(n, seed, False, "keyed")
    tied = _frame(np.full(reps, TIE_BAIT), np.full(reps, TIE_OE), rng, na=0.0)
    other = _frame([TIE_BAIT2], [TIE_OE], rng, na=0.0)
    if not scattered:
        x = pd.concat([base.iloc[:1000], other, tied, base.iloc[1000:]], ignore_index=True)
        return x, 1001
    pos = np.sort(rng.choice(n + reps + 1, reps + 1, replace=False))
    x = pd.concat([base, tied, other], ignore_index=True)
    slot = np.empty(len(x), dtype=np.int64)
    rest = np.setdiff1d(np.arange(len(x)), pos)
    slot[rest] = np.arange(n)                                   # base rows keep their order
    slot[pos[1:]] = n + np.arange(reps)                         # the tied rows, in their own order, at the drawn positions
    slot[pos[0]] = n + reps                                     # the larger bait's row in front of them all
    return x.iloc[slot].reset_index(drop=True), int(pos[1])


NA_BAIT = ID_MIN + 3150


@functools.lru_cache(maxsize=None)
def na_winner(n=4097, seed=4):
    """table(n) plus (a) bait NA_BAIT whose winning row — the smallest other end, placed LAST in the table — has NaN s_j and NA tblb
    while its other rows, in front, have values; (b) one row with the smallest (baitID, otherEndID) of the table, a bait outside
    the map, codes (LEVB[0], LEVL[0]) and NaN Tmean: it wins that pair.  nid = 3200."""
    import pandas as pd
    rng = np.random.default_rng(seed)
    base = table(n, seed, False, "shuffled")
    late = _frame(np.full(6, NA_BAIT), NA_BAIT + np.array([9, 8, 7, 6, 5, 1]), rng, na=0.0)
    late.loc[5, "s_j"], late.loc[5, "tblb"] = np.nan, None
    first = _frame([ID_MIN - 50], [ID_MIN - 60], rng, na=0.0)
    first["tblb"], first["tlb"], first["Tmean"] = LEVB[0], LEVL[0], np.nan
    return pd.concat([base.iloc[:2000], first, base.iloc[2000:], late], ignore_index=True)


@functools.lru_cache(maxsize=None)
def not_a_function(n=4097, seed=6):
    """table(n) with ONE row's refBinMean changed: its distbin now carries two values."""
    x = table(n, seed, False, "shuffled").copy()
    k = int(np.flatnonzero((x["distbin"] == "bin003").to_numpy() & x["refBinMean"].notna().to_numpy())[1])
    x.loc[k, "refBinMean"] = 0.123
    return x


def twin_keeping(keep):
    """pipeline.background_tables with every ``keep="first"`` replaced by ``keep`` (the source text itself, re-executed)."""
    import inspect

    from chicdiff_amd import pipeline
    src = inspect.getsource(pipeline.background_tables)
    assert src.count('keep="first"') == 3
    ns = dict(vars(pipeline))
    exec(src.replace('keep="first"', f'keep="{keep}"'), ns)
    return ns["background_tables"]


def same_bits(a, b):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    na = np.isnan(a)
    return a.shape == b.shape and np.array_equal(na, np.isnan(b)) and np.array_equal(a[~na].view(np.int64), b[~na].view(np.int64))
