"""Small inputs of the region stage with the edge cases planted; every builder returns what it planted (``planted``: name -> rows),
and tests/test_region_twin.py asserts that each case reaches what it is for.  These are the smallest shapes at which the kernels can go
wrong: one block, a block edge either side, more than one block, and for the grid strides one case each past the launch's grid.

No case here may reach a device whose region-universe kernels form the window in 32 bits: the extreme IDs are rows of the universe
cases from the start (see ru_window.h)."""
import functools

import numpy as np

INT32_MIN, INT32_MAX = -2 ** 31, 2 ** 31 - 1
EXTREMES = [INT32_MIN, INT32_MIN + 1, INT32_MIN + 40, INT32_MAX - 40, INT32_MAX - 2, INT32_MAX - 1, INT32_MAX]

# ---- region universe --------------------------------------------------------------------------------------------------------
MAXFRAG = 3000
CHR_ENDS = (1200, 2100, MAXFRAG)                                  # three chromosomes: 1..1200, 1201..2100, 2101..3000
HOLES = [300, 320] + list(range(700, 791)) + [1500, 2600]         # IDs the map does not hold
UNIVERSE_N = (1, 255, 256, 257, 513)
UNIVERSE_S = (0, 1, 5, 15, 16, 17, 20, 40)
BAIT = 600                                                        # the bait of the planted chromosome-0 peaks


def small_map():
    ids = np.arange(MAXFRAG + 1)
    chr_of = np.where(ids <= CHR_ENDS[0], 0, np.where(ids <= CHR_ENDS[1], 1, 2)).astype(np.int32)
    chr_of[0] = -1
    chr_of[HOLES] = -1
    return chr_of


def planted_peaks(s):
    """(name, bait, oe) of every planted edge at RUexpand = s."""
    B, P = BAIT, []
    add = lambda name, b, o: P.append((name, int(b), int(o)))
    add("dist_s1_right", B, B + s + 1)            # distance exactly s + 1: the window stops two short of the bait
    add("dist_s2_right", B, B + s + 2)            # s + 2: the full window, which ends right beside the bait's neighbour
    add("dist_s1_left", B, B - s - 1)
    add("dist_s2_left", B, B - s - 2)
    add("beside_right", B, B + 1)                 # RUexpand = 0: (bait + 2):(oe + 0) counts DOWN: two rows
    add("beside_left", B, B - 1)
    if s >= 16:                                   # windows of 31, 32, 33 candidates beside the wide ones: mask and walk in one launch
        for w in (31, 32, 33):
            d = w + 1 - s                         # (bait + 2):(oe + s) holds d + s - 1 IDs
            if 1 <= d <= s + 1:
                add(f"w{w}_near", B, B + d)
            add(f"w{w}_end", 2500, MAXFRAG + s + 1 - w)    # (oe - s):maxfrag holds maxfrag - oe + s + 1 IDs
            add(f"w{w}_start", B, w - s)                   # 1:(oe + s) holds oe + s IDs
    add("straddle_1", B, 3)
    add("straddle_maxfrag", 2500, MAXFRAG - 2)
    add("straddle_chr", B, CHR_ENDS[0] - 1)
    add("oe_other_chr", B, CHR_ENDS[0] + 3)
    add("hole_first", 1000, 300 + s)
    add("hole_last", 1000, 320 - s)
    add("hole_every", 1000, 745)
    add("bait_off_map", MAXFRAG + 50, MAXFRAG - 3)
    add("bait_on_hole", 750, 900)
    add("bait_zero", 0, 5)
    add("bait_negative", -7, 3)
    add("bait_above", MAXFRAG + 1, MAXFRAG - 1)
    for e in EXTREMES:
        add("extreme", 100, e)
        add("extreme", e, 100)
        add("extreme", e, e + 1 if e < 0 else e - 1)
    add("extreme", INT32_MIN, INT32_MAX)
    add("extreme", INT32_MAX, INT32_MIN)
    return P


def _filler(rng, m):
    good = np.setdiff1d(np.arange(50, MAXFRAG - 50), HOLES)
    b = rng.choice(good, m)
    return b, b + rng.integers(1, 46, m) * rng.choice([-1, 1], m)


@functools.lru_cache(maxsize=None)
def universe_case(n, s, seed=0):
    """n peaks at RUexpand = s on small_map(): normal peaks with the planted edges between them (odd rows).  n = 513: regions 256 .. 511
    are all empty, so the second block of the fill owns no row.  n = 255, 257: an empty first and an empty last region.  n = 1: one
    planted peak, which one depends on s and seed."""
    rng = np.random.default_rng(1000 * n + 10 * s + seed)
    P = planted_peaks(s)
    planted = {}
    if n == 1:
        name, b, o = P[(7 * UNIVERSE_S.index(s) + seed) % len(P)] if s in UNIVERSE_S else P[seed % len(P)]
        bait, oe = np.array([b]), np.array([o])
        planted[name] = [0]
    else:
        bait, oe = _filler(rng, n)
        assert 2 * len(P) < 255
        for k, (name, b, o) in enumerate(P):
            bait[2 * k + 1], oe[2 * k + 1] = b, o
            planted.setdefault(name, []).append(2 * k + 1)
        if n in (255, 257):
            bait[0], oe[0] = 0, 5
            bait[n - 1], oe[n - 1] = -7, 3
            planted["empty_first"], planted["empty_last"] = [0], [n - 1]
        if n > 512:
            empties = [(b, o) for name, b, o in P if name.startswith(("bait_", "extreme"))]
            for i in range(256, 512):
                bait[i], oe[i] = empties[i % len(empties)]
            bait[512], oe[512] = BAIT, BAIT + 40
            planted["empty_run"] = list(range(256, 512))
    return dict(bait=bait.astype(np.int32), oe=oe.astype(np.int32), chr_of=small_map(), s=s, planted=planted)


@functools.lru_cache(maxsize=None)
def universe_all_empty(n=257, s=5):
    """every region empty: total = 0"""
    empties = [(b, o) for name, b, o in planted_peaks(s) if name.startswith(("bait_", "extreme", "hole_every"))]
    rows = [empties[i % len(empties)] for i in range(n)]
    return dict(bait=np.array([b for b, _ in rows], np.int32), oe=np.array([o for _, o in rows], np.int32), chr_of=small_map(), s=s,
                planted={"all_empty": list(range(n))})


def universe_cases():
    return [universe_case(n, s) for n in UNIVERSE_N for s in UNIVERSE_S] + [universe_case(1, 5, seed) for seed in (1, 2, 3)] + [universe_all_empty()]


def refusal_cases(s=5, n=300):
    """baitID == oeID at row 0, a middle row, the last row, and at the largest ID: (name, bait, oe, chr_of, s, row)"""
    out = []
    for name, row, v in (("first", 0, 7), ("middle", n // 2 + 1, BAIT), ("last", n - 1, MAXFRAG + 9), ("extreme", 257, INT32_MAX), ("lowest", 3, INT32_MIN)):
        c = universe_case(n, s, seed=5)
        bait, oe = c["bait"].copy(), c["oe"].copy()
        bait[row] = oe[row] = v
        out.append((name, bait, oe, c["chr_of"], s, row))
    return out


UNIVERSE_STRIDE_N = 4096 * 256 + 1   # one region more than the grid of the count and fill launches covers in one pass


@functools.lru_cache(maxsize=None)
def universe_stride_case(s=5):
    """n = 4096 * 256 + 1: the small cases' peaks drawn again and again, so that every block meets planted edges"""
    rng = np.random.default_rng(77)
    c = universe_case(513, s)
    idx = rng.integers(0, 513, UNIVERSE_STRIDE_N)
    idx[-1] = 1   # the one region of the second pass is a planted, non-empty one (dist_s1_right)
    return dict(bait=c["bait"][idx].copy(), oe=c["oe"][idx].copy(), chr_of=c["chr_of"], s=s, planted={"second_pass": [UNIVERSE_STRIDE_N - 1]})


# ---- key table --------------------------------------------------------------------------------------------------------------
KEY_ROWS = (1, 2047, 2048, 2049, 70001)
KEY_STRIDE_ROWS = 2048 * 2048 + 1   # one row more than the key kernel's grid covers in one pass
KEY_MAX_ID = 300


@functools.lru_cache(maxsize=None)
def key_table_case(nrows, flags_mode, seed=0):
    """nrows unique (baitID, otherEndID, N) rows in random order; ``flags_mode``: "given", "zero" (an empty table) or "absent".
    Planted: baits that are negative, above max_id and INT32_MAX; otherEndID negative and at both int32 ends; N 0, negative and INT32_MAX."""
    rng = np.random.default_rng(31 * nrows + seed)
    nb = KEY_MAX_ID + 41
    K = max(64, -(-2 * nrows // nb))
    idx = rng.permutation(nb * K)[:nrows]
    bait, oe = idx // K, idx % K + 1
    N = rng.integers(1, 50, nrows)
    specials = [("oe_negative", 5, -1, 13), ("bait_negative", -1, 5, 7), ("bait_int32_max", INT32_MAX, 9, 11), ("oe_int32_min", 5, INT32_MIN, 14),
                ("oe_int32_max", 5, INT32_MAX, 15), ("N_zero", 6, -2, 0), ("N_negative", 7, K + 5, -4), ("N_int32_max", 8, K + 6, INT32_MAX),
                ("bait_int32_min", INT32_MIN, 1, 3), ("bait_int32_max_oe_negative", INT32_MAX, -1, 12), ("zero_zero", 0, 0, 1),
                ("bait_above_max_id", KEY_MAX_ID + 1, 0, 21)]
    planted = {}
    for k, (name, b, o, v) in enumerate(specials[: max(1, min(len(specials), nrows // 8))]):
        row = (k * nrows) // len(specials) if nrows > 1 else 0
        bait[row], oe[row], N[row] = b, o, v
        planted[name] = [row]
    if flags_mode == "given":
        flags = (rng.random(KEY_MAX_ID + 1) < 0.6).astype(np.uint8)
        flags[[0, 5, 6, 7, 8]] = 1
    elif flags_mode == "zero":
        flags = np.zeros(KEY_MAX_ID + 1, dtype=np.uint8)
    else:
        assert flags_mode == "absent"
        flags = None
    return dict(bait=bait.astype(np.int32), oe=oe.astype(np.int32), N=N.astype(np.int32), flags=flags, planted=planted)


def key_table_cases():
    return [key_table_case(n, m) for n in KEY_ROWS for m in ("given", "absent")] + [key_table_case(2049, "zero"), key_table_case(1, "zero")]


def key_table_repeats():
    """Repeated pairs (outside what the joins are written for): count_table keeps them in file order, each with its own N."""
    bait = np.array([4, 2, 4, 4, 2, 9, 4, 2, 4], dtype=np.int32)
    oe = np.array([7, 1, 7, -3, 1, 0, 7, 1, -3], dtype=np.int32)
    return dict(bait=bait, oe=oe, N=np.arange(10, 19, dtype=np.int32), flags=None, planted={"repeat": [0, 2, 6]})


# ---- joins ------------------------------------------------------------------------------------------------------------------
JOIN_S = (1, 2, 3, 8, 64)
JOIN_NRU = (1, 255, 256, 257)
JOIN_STRIDE_NRU = 8192 * 256 + 1   # one row more than the inner join's grid covers in one pass


def _pack(b, o):
    return (int(b) << 32) | (int(o) & 0xFFFFFFFF)


@functools.lru_cache(maxsize=None)
def join_case(S, nru, variant="normal", seed=0):
    """S key tables (as {(bait, oe): N} in ``dicts`` and as sorted (keys, vals) in ``tables``) and nru query rows.  ``variant``:
    "normal"; "one_empty" (table S // 2 holds nothing: every inner-join output is 0); "one_key" (every table holds the one pair (5, 9)).
    Planted pairs: "first" / "last" = the smallest / largest key of every table; "zero_hit": held by all, N = 0 in table 0;
    "all_but_first" / "all_but_middle" / "all_but_last"; queries "below" and "above" every key (negative baits included)."""
    rng = np.random.default_rng(100 * S + nru + seed)
    base = sorted({(int(b), int(o)) for b, o in zip(rng.integers(1, 41, 2500), rng.integers(-5, 201, 2500))})
    dicts = []
    for t in range(S):
        if variant == "one_key":
            d = {(5, 9): t + 1}
        else:
            d = {p: int(v) for p, v, k in zip(base, rng.integers(1, 50, len(base)), rng.random(len(base))) if k < 0.8}
            d[(0, 0)] = 100 + t
            d[(50, -1)] = 200 + t
            d[(10, 300)] = 0 if t == 0 else 300 + t
            if t != 0:
                d[(11, 300)] = 400 + t
            if t != S // 2:
                d[(12, 300)] = 500 + t
            if t != S - 1:
                d[(13, 300)] = 600 + t
            if variant == "one_empty" and t == S // 2:
                d = {}
        dicts.append(d)
    tables = []
    for d in dicts:
        items = sorted((_pack(b, o), v) for (b, o), v in d.items())
        tables.append((np.array([k for k, _ in items], dtype=np.int64), np.array([v for _, v in items], dtype=np.int32)))
    named = [("first", (0, 0)), ("last", (50, -1)), ("zero_hit", (10, 300)), ("all_but_first", (11, 300)), ("all_but_middle", (12, 300)),
             ("all_but_last", (13, 300)), ("below", (-3, 7)), ("below", (INT32_MIN, 0)), ("above", (51, 0)), ("above", (INT32_MAX, INT32_MAX)),
             ("between", (0, -1)), ("one_key", (5, 9)), ("below", (-1, -1)), ("above", (50, 0)) if variant == "one_key" else ("between", (49, 0))]
    q, planted = [], {}
    for k in range(nru):
        if k < 3 * len(named) and k % 3 == (seed % 3) or nru == 1:
            name, pair = named[(k // 3 + seed) % len(named)]
            planted.setdefault(name, []).append(k)
            q.append(pair)
        elif rng.random() < 0.7:
            q.append(base[rng.integers(0, len(base))])
        else:
            q.append((int(rng.integers(-2, 53)), int(rng.integers(-8, 320))))
    return dict(qbait=np.array([b for b, _ in q], dtype=np.int32), qoe=np.array([o for _, o in q], dtype=np.int32), tables=tables, dicts=dicts,
                planted=planted, S=S, variant=variant)


def join_cases():
    out = [join_case(S, nru) for S in JOIN_S for nru in JOIN_NRU]
    out += [join_case(3, 257, "one_empty"), join_case(1, 255, "one_empty"), join_case(3, 257, "one_key"), join_case(8, 1, "normal", 1),
            join_case(2, 1, "normal", 2)]
    return out


def tile_rows(m, n, seed):
    """n row numbers into a case of m rows: every row at least once when n >= m, the last one row 0"""
    rng = np.random.default_rng(seed)
    idx = rng.integers(0, m, n)
    idx[: min(m, n)] = np.arange(min(m, n))
    idx[-1] = 0
    return idx


# ---- avDist -----------------------------------------------------------------------------------------------------------------
AVDIST_N = (1, 255, 256, 257)
AVDIST_STRIDE_N = 4096 * 256 + 1
AV_ID_MIN, AV_NID = 11, 400
AV_KINDS = ("normal", "empty", "off_map_all", "off_map_one", "trans", "negative_code", "single", "long")


def avdist_map():
    """midsum = start + end per ID (all four residues mod 4, so round(x.5) goes both ways; midpoints up to 5e8) and chromosome codes
    (two chromosomes, the last ten IDs with a code below zero = not on the map)"""
    k = np.arange(AV_NID, dtype=np.int64)
    midsum = 2_500_000 * k + (k % 4) + 1000
    chr_codes = np.where(k < 250, 0, np.where(k < 390, 1, -1)).astype(np.int32)
    return midsum, chr_codes


@functools.lru_cache(maxsize=None)
def avdist_case(n, with_chr, seed=0):
    """n regions over CSR-ordered RU rows; region i is of kind AV_KINDS[(i + seed) % 8].  Every region has fewer than 1 024 rows."""
    rng = np.random.default_rng(17 * n + seed + (1000 if with_chr else 0))
    midsum, chr_codes = avdist_map()
    lo, hi = AV_ID_MIN, AV_ID_MIN + AV_NID - 1
    rb, ro, ptr, planted = [], [], [0], {}
    for i in range(n):
        kind = AV_KINDS[(i + seed) % len(AV_KINDS)]
        planted.setdefault(kind, []).append(i)
        b = int(rng.integers(lo + 40, lo + 200))                       # a chromosome-0 bait
        m = {"empty": 0, "single": 1, "long": 200}.get(kind, int(rng.integers(2, 31)))
        o0 = b + int(rng.integers(-35, 6))
        oes = [o for o in range(o0, o0 + m + 1) if o != b][:m]          # both signs of the distance
        baits = [b] * m
        if kind == "long":
            oes = [lo + 5 + k for k in range(230) if lo + 5 + k != b][:m]   # 200 rows, all on chromosome 0
        if kind == "off_map_all":
            off = [lo - 1, hi + 1, 0, -5, 10 ** 9, INT32_MAX]
            if i % 2:
                baits = [off[(i + k) % len(off)] for k in range(m)]
            else:
                oes = [off[(i + k) % len(off)] for k in range(m)]
        elif kind == "off_map_one":
            oes[m // 2] = (hi + 1, lo - 1, -5)[i % 3]
        elif kind == "trans":
            oes[m - 1] = lo + 300                                       # chromosome 1 among chromosome-0 rows (NA only when chr is given)
        elif kind == "negative_code":
            oes[0] = hi - 3                                             # code below zero: dropped when chr is given, a far row otherwise
        rb += baits
        ro += oes
        ptr.append(len(rb))
    return dict(ru_bait=np.array(rb, dtype=np.int32).reshape(-1), ru_oe=np.array(ro, dtype=np.int32).reshape(-1), region_ptr=np.array(ptr, dtype=np.int64),
                id_min=AV_ID_MIN, midsum=midsum, chr=chr_codes if with_chr else None, planted=planted)


def avdist_cases():
    return [avdist_case(n, c) for n in AVDIST_N for c in (False, True)] + [avdist_case(1, True, seed) for seed in (1, 2, 3, 4, 5, 6, 7)]
