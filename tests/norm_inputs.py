"""Small seeded inputs of the normalisation stage (fragment background a3, window sums a2, size factors a5, offsets a4) with the edges
planted, for tests/test_norm_twin.py (the CPU oracle under tests/norm_twin.py) and tests/test_gpu_norm.py (the kernels under it).
At most ~3 000 RU rows, ~600 regions and S <= 20 per case: the 50-digit twin then takes seconds.

Geometry: the first 3 000 chr19 HindIII fragments of the reference's restriction map and the baits among them (tests/golden/), laid
out as tests/test_oracle.py::_a3_inputs lays them out.  Every case carries `planted`: name -> row indices, which the CPU test asserts
to be present and to be what they are called."""
import os

import mpmath as mp
import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
NA_INT = np.iinfo(np.int32).min


def geometry():
    rmap = np.loadtxt(os.path.join(HERE, "golden", "chr19_HindIII_first3000.rmap"), dtype=str)
    start, end, ids = rmap[:, 1].astype(np.int64), rmap[:, 2].astype(np.int64), rmap[:, 3].astype(np.int64)
    baits = np.loadtxt(os.path.join(HERE, "golden", "chr19_baitIDs_first3000.txt"), dtype=np.int64)
    assert np.array_equal(ids, np.arange(ids[0], ids[0] + len(ids)))
    return int(ids[0]), len(ids), (start + end).astype(np.int64), baits


def _dist(midsum, b, o):
    """round((midsum[o] - midsum[b]) / 2), halves to even, in integers"""
    d2 = int(midsum[o]) - int(midsum[b])
    q, r = divmod(d2, 2)
    return q if r == 0 or q % 2 == 0 else q + 1


def _params(fit, omin, omax):
    """the ten distance-function parameters of one replicate: the lines continue the cubic with its value and slope (chicdiff.R:565-566),
    formed at 50 digits and rounded once, so that the continuity holds to the last bit of alpha and beta"""
    with mp.workdps(50):
        c = [mp.mpf(float(v)) for v in fit]
        out = [float(v) for v in fit]
        for t in (mp.mpf(float(omin)), mp.mpf(float(omax))):
            beta = c[1] + 2 * c[2] * t + 3 * c[3] * t * t
            alpha = c[0] + (c[1] - beta) * t + c[2] * t * t + c[3] * t ** 3
            out += [float(alpha), float(beta)]
        return out + [float(omin), float(omax)]


A3_S = [1, 4, 8, 16, 20]


def a3_case(S, seed=0, rows_per_bait=30, nbaits=50, with_off_map=True):
    id_min, nid, midsum, baits = geometry()
    rng = np.random.default_rng(100 * seed + S)
    ib = baits - id_min                                           # indices of the baits
    planted = {}
    rows = []                                                     # (bait index, other-end index), off-map indices allowed

    def plant(name, pairs):
        planted[name] = list(range(len(rows), len(rows) + len(pairs)))
        rows.extend(pairs)

    use = ib[5:5 + nbaits]
    bb = np.repeat(use, rows_per_bait)
    oo = bb + rng.integers(-60, 61, len(bb))
    keep = (oo != bb) & (oo >= 0) & (oo < nid)
    plant("bulk", list(zip(bb[keep].tolist(), oo[keep].tolist())))
    plant("neighbours", [(int(b), int(b) + d) for b in use[:8] for d in (-1, 1)])
    plant("dist 0", [(int(use[0]), int(use[0])), (int(use[7]), int(use[7]))])
    far = [(int(b), int(o)) for b in use[:6] for o in (int(b) + 450, int(b) + 900) if o < nid]
    plant("far", far)
    plant("map ends", [(int(ib[0]), 0), (int(ib[-1]), nid - 1), (int(ib[0]), nid - 1)])
    # odd midpoint differences: d2 = 1 mod 4 rounds down to the even q, d2 = 3 mod 4 up to the even q + 1; both signs.  And pairs
    # whose midpoints are both odd with midsum[o] = 1, midsum[b] = 3 mod 4: rounding the midpoints first (:871) loses 1
    want = {"odd down +": lambda d2, mo, mb: d2 > 0 and d2 % 4 == 1, "odd up +": lambda d2, mo, mb: d2 > 0 and d2 % 4 == 3,
            "odd down -": lambda d2, mo, mb: d2 < 0 and d2 % 4 == 1, "odd up -": lambda d2, mo, mb: d2 < 0 and d2 % 4 == 3,
            "midpoints rounded apart": lambda d2, mo, mb: mo % 4 == 1 and mb % 4 == 3}
    for name, test in want.items():
        found = []
        for b in use:
            for d in list(range(2, 40)) + list(range(-2, -40, -1)):
                o = int(b) + d
                if 0 <= o < nid and test(int(midsum[o]) - int(midsum[b]), int(midsum[o]), int(midsum[b])):
                    found.append((int(b), o))
                    break
            if len(found) == 4:
                break
        plant(name, found)
    # Tmean lookups: a tblb row partly NaN (2), one all NaN (4), the cell (2, 3) NaN; other ends without a tlb
    bA, bB, bC = int(use[10]), int(use[11]), int(use[12])
    oX, oY, oZ = bA + 7, bA + 9, bA + 11
    plant("tlb missing, tblb partly NaN", [(bA, oX)])
    plant("tlb missing, tblb all NaN", [(bB, oX)])
    plant("cell NaN", [(bA, oY)])
    plant("cell seen", [(bA, oZ), (bB, oZ)])
    plant("s_j NaN, tblb set", [(bC, oX), (bC, oZ)])
    sI = int(use[13]) + 5
    plant("s_i NaN", [(int(use[13]), sI), (bA, sI)])
    # ld at obs.min / obs.max: the edge pair of each end; obs.min / obs.max are set from them below
    lo_pair = min(((int(b), int(b) + d) for b in use[20:30] for d in range(1, 6)), key=lambda p: abs(abs(_dist(midsum, *p)) - 10000))
    hi_pair = min(((int(b), int(b) + d) for b in use[20:30] for d in range(100, 200) if int(b) + d < nid),
                  key=lambda p: abs(abs(_dist(midsum, *p)) - 1500000))
    plant("at obs.min", [lo_pair])
    plant("at obs.max", [hi_pair])
    if with_off_map:
        plant("off map", [(-1, int(use[0])), (int(use[0]), nid), (int(use[1]), -5), (nid + 3, int(use[1]) + 2), (-1, nid)])
    bait = np.array([id_min + b for b, _ in rows], dtype=np.int32)
    oe = np.array([id_min + o for _, o in rows], dtype=np.int32)

    sj = np.full((S, nid), np.nan)
    sj[:, ib] = np.exp(rng.normal(0, 0.3, (S, len(ib))))
    si = np.where(rng.random((S, nid)) < 0.8, np.exp(rng.normal(0, 0.3, (S, nid))), np.nan)
    ntblb, ntlb = 5, 6
    tblb = np.full((S, nid), -1, dtype=np.int32)
    tblb[:, ib] = rng.integers(0, ntblb - 1, (S, len(ib)))            # the last row of T (all NaN) is left to the planted bait
    gone = ib[::17]
    gone = gone[~np.isin(gone, [bA, bB, bC, use[0], use[7], lo_pair[0], hi_pair[0]])]
    sj[:, gone] = np.nan                                          # baits Chicago filtered out: s_j NA, and no tblb either
    tblb[:, gone] = -1
    tlb = np.where(rng.random((S, nid)) < 0.85, rng.integers(0, ntlb, (S, nid)), -1).astype(np.int32)
    T = np.exp(rng.normal(-3, 0.5, (S, ntblb, ntlb)))
    T[:, 2, 3] = np.nan
    T[:, 2, 0] = np.nan
    T[:, 4, :] = np.nan
    T[:, 1, 5] = T[:, 3, :].min(axis=1) / 8                        # the lowest cell of the whole table sits in row 1: not row 2's lowest
    tblb[:, bA], tblb[:, bB], tblb[:, bC] = 2, 4, 1
    sj[:, bC] = np.nan                                            # s_j NA with a tblb: Bmean NA, Tmean stays
    tlb[:, oX], tlb[:, oY], tlb[:, oZ] = -1, 3, 1
    for k, (b, _) in enumerate([rows[i] for i in planted["dist 0"]]):
        tblb[:, b], tlb[:, b] = (0, 3)[k], 1                      # a Tmean that was observed: FullMean = Inf + Tmean
    si[:, sI] = np.nan
    si[:, [lo_pair[1], hi_pair[1]]] = np.exp(rng.normal(0, 0.3, (S, 2)))
    for b, _ in [rows[i] for i in planted["dist 0"]]:
        si[:, b] = np.exp(rng.normal(0, 0.3, S))                  # Inf * s_i, not Inf * NA -> 1
    lmin = float(np.log(float(abs(_dist(midsum, *lo_pair)))))
    lmax = float(np.log(float(abs(_dist(midsum, *hi_pair)))))
    distfun = np.zeros((S, 10))
    edge = []
    for s in range(S):
        k = (s + seed + S) % 3                                    # the double log itself, one ulp above it, one ulp below it
        step = [0.0, np.inf, -np.inf][k]
        omin = lmin if k == 0 else float(np.nextafter(lmin, step))
        omax = lmax if k == 0 else float(np.nextafter(lmax, -step))
        edge.append(["equal", "one ulp off (a)", "one ulp off (b)"][k])
        distfun[s] = _params([14.0 + 0.2 * s, -1.6, 0.05, -0.003], omin, omax)
    return dict(args=dict(bait=bait, oe=oe, id_min=id_min, midsum=midsum, sj=sj, si=si, tblb=tblb, tlb=tlb, T=T, distfun=distfun),
                planted=planted, rows=rows, S=S, edge=edge, lmin=lmin, lmax=lmax)


# ---------------------------------------------------------------------------------------------------------------------------
# a2
# ---------------------------------------------------------------------------------------------------------------------------
WIN_CAP = 3072   # kWinCap: fragments a block of 256 regions stages; beyond it the block takes the direct path
A2_CASES = ["blocks", "one long region", "n1", "n255", "n256", "n257"]


def a2_case(name):
    rng = np.random.default_rng(sum(map(ord, name)))
    planted = {}
    if name == "blocks":
        S = 4
        ragged = lambda k: [1 + (i % 11) for i in range(k)]
        sizes = [0, 0, 0] + ragged(200) + [0, 0, 0, 0] + ragged(23) + [13] * 300 + ragged(60) + [0, 0] + ragged(26) + [0, 0]
        assert sizes[230:530] == [13] * 300
    elif name == "one long region":
        S = 3
        sizes = [3, 0, 4000] + [1 + (i % 11) for i in range(253)] + [5]          # n = 257: the last region alone in its block
    else:
        n = int(name[1:])
        S = {1: 1, 255: 20, 256: 8, 257: 17}[n]
        sizes = [int(v) for v in rng.integers(0, 12, n)]
        if n == 1:
            sizes = [7]
    ptr = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)
    n, nfrag = len(sizes), int(ptr[-1])
    fm = np.exp(rng.normal(-1, 1, (nfrag, S)))
    fn = rng.integers(0, 50, (nfrag, S)).astype(np.int32)
    size_at = lambda k: [i for i, v in enumerate(sizes) if v >= k]
    if n > 20:
        cand = size_at(6)
        r_nan, r_inf, r_both, r_wide, r_wide2 = cand[1], cand[3], cand[5], cand[7], cand[-2]
        fm[ptr[r_nan] + 2, :] = np.nan
        fm[ptr[r_inf] + 1, 0] = np.inf
        fm[ptr[r_both] + 0, -1] = np.inf
        fm[ptr[r_both] + 3, -1] = np.nan
        for r in (r_wide, r_wide2):                                   # twelve orders of magnitude inside one region
            k = sizes[r]
            fm[ptr[r]:ptr[r + 1], :] = 10.0 ** np.linspace(-6, 6, k)[rng.permutation(k)][:, None] * rng.uniform(1, 2, (k, S))
        planted.update(nan=[r_nan], inf=[r_inf], inf_and_nan=[r_both], wide=[r_wide, r_wide2])
        if name == "blocks":
            fm[ptr[300] + 5, 1] = np.nan                              # inside the direct-path block too
            fm[ptr[301] + 5, 2] = np.inf
            fm[ptr[302]:ptr[303], :] = 10.0 ** np.linspace(-6, 6, 13)[:, None] * rng.uniform(1, 2, (13, S))
            planted.update(direct_nan=[300], direct_inf=[301], direct_wide=[302])
        if name == "one long region":
            fm[ptr[2]:ptr[3], 1] = 10.0 ** rng.uniform(-6, 6, 4000)
    planted["empty"] = [i for i, v in enumerate(sizes) if v == 0]
    direct = [k for k in range((n + 255) // 256) if ptr[min(256 * (k + 1), n)] - ptr[256 * k] > WIN_CAP]
    return dict(fragN=fn, fragFM=fm, region_ptr=ptr, n=n, S=S, sizes=sizes, planted=planted, direct_blocks=direct, nblocks=(n + 255) // 256)


# ---------------------------------------------------------------------------------------------------------------------------
# a5
# ---------------------------------------------------------------------------------------------------------------------------
def a5_cases():
    import test_size_factors_direct as sfd
    rng = np.random.default_rng(29)
    c = {}
    one = np.zeros((10, 4), dtype=np.int32)
    one[rng.integers(0, 10, 12), rng.integers(0, 4, 12)] = 7
    one[:, 0] = 0
    one[6] = [3, 50, 7, 11]
    c["one used row"] = one
    two = one.copy()
    two[2] = [30, 5, 70, 2]
    c["two used rows"] = two
    c["odd 1001x5"] = (rng.poisson(30.0, (1001, 5)) + 1).astype(np.int32)
    c["even 1000x9"] = (rng.poisson(30.0, (1000, 9)) + 1).astype(np.int32)
    c["one sample"] = (rng.poisson(30.0, (300, 1)) + 1).astype(np.int32)
    c["400x16"] = (rng.poisson(8.0, (400, 16))).astype(np.int32)            # zeros drop about a tenth of the rows
    c["257x8"] = (rng.poisson(100.0, (257, 8)) + 1).astype(np.int32)
    c["split_middles"] = sfd.split_middles()[:5000]
    c["zeros_and_negatives"] = sfd.zeros_and_negatives()[:5000]
    col = np.random.default_rng(3).poisson(40.0, 3001).astype(np.int32) + 1
    c["equal_columns"] = np.stack([col, col], 1)
    ties = (rng.poisson(30.0, (3001, 4)) + 1).astype(np.int32)
    ties[:2050] = [10, 20, 30, 41]
    c["ties 3001x4"] = np.ascontiguousarray(ties[rng.permutation(3001)])
    c["column_x1000000"] = sfd.scaled(1000000)[:3000]
    big = rng.integers(1, 2 ** 31, (501, 8)).astype(np.int64)
    big[:40] = rng.integers(1, 1000, (40, 8))
    big[7, 3] = big[100, 0] = 2 ** 31 - 1
    c["up to 2^31-1"] = big.astype(np.int32)
    assert all(v.shape[0] <= 5000 and v.dtype == np.int32 for v in c.values())
    return c


# ---------------------------------------------------------------------------------------------------------------------------
# a4
# ---------------------------------------------------------------------------------------------------------------------------
A4_SHAPES = [(2, 1030), (3, 255), (4, 257), (5, 1), (8, 1030), (9, 255), (12, 257), (16, 1030), (17, 1030), (17, 1), (20, 257)]   # (S, n)
THETAS = [None, 0.0, 0.25, 0.5, 1.0]


def a4_case(S, n):
    rng = np.random.default_rng(1000 * S + n)
    fm = np.exp(rng.normal(0, 1, (n, S))) * np.exp(rng.normal(-2, 2, (n, 1)))
    planted = {}
    if n == 1:
        if S > 16:
            fm[0, 0] = np.nan
            planted["NaN first column"] = [0]
    else:
        L = S - 1
        spots = {"NaN first column": (0, 0, np.nan), "zero last column": (1, L, 0.0), "negative first column": (2, 0, -1.5), "Inf last column": (3, L, np.inf),
                 "Inf first column": (n - 1, 0, np.inf), "negative last column": (n - 2, L, -2.0), "zero first column": (n - 3, 0, 0.0),
                 "NaN last column": (n - 4, L, np.nan)}
        for name, (r, j, v) in spots.items():
            fm[r, j] = v
            planted[name] = [r]
        fm[10] = 0.3728
        planted["equal values"] = [10]
        fm[11:21] = 10.0 ** rng.uniform(-30, 30, (10, S))
        fm[11, 0], fm[11, L] = 1e-30, 1e30
        planted["wide"] = list(range(11, 21))
    sf = np.exp(rng.normal(0, 0.3, S)) * 1.7
    assert abs(np.log(sf).mean()) > 1e-3                          # geometric mean not 1: a renormalised NA row shows
    return dict(fm=fm, sf=sf, S=S, n=n, planted=planted)


# ---------------------------------------------------------------------------------------------------------------------------
# the chain a3 -> a2 -> a4 on one small region set
# ---------------------------------------------------------------------------------------------------------------------------
def chained_case():
    """RU rows in region order (the rows of a3_case(4) without the off-map ones, cut into regions of 1 .. 11 rows), a count table per
    replicate ((baitID << 32 | otherEndID) -> N, sorted, as tests/assemble_inputs.py builds them) and the counts they give every row."""
    a = a3_case(4, seed=3, rows_per_bait=12, nbaits=40, with_off_map=False)
    args = a["args"]
    nru = len(args["bait"])
    rng = np.random.default_rng(41)
    zero_row = a["planted"]["dist 0"][0]
    cuts = {0, nru, zero_row, zero_row + 1}                           # the dist = 0 row is a region of its own: its sum is +Inf, not NaN
    at = 0
    while at < nru:
        cuts.add(at)
        at += int(rng.integers(1, 12))
    ptr = np.array(sorted(cuts), dtype=np.int64)
    sizes = np.diff(ptr).tolist()
    key = (args["bait"].astype(np.int64) << 32) | args["oe"].astype(np.int64)
    uniq = np.unique(key)
    tables, fragN = [], np.zeros((nru, 4), dtype=np.int32)
    for s in range(4):
        keep = rng.random(len(uniq)) < 0.9
        ks, vs = uniq[keep], rng.integers(1, 50, int(keep.sum())).astype(np.int32)
        tables.append((ks, vs))
        pos = np.searchsorted(ks, key)
        hit = (pos < len(ks)) & (ks[np.minimum(pos, len(ks) - 1)] == key)
        fragN[hit, s] = vs[pos[hit]]
    region = int(np.searchsorted(ptr, zero_row, side="right") - 1)
    return dict(a3=a, region_ptr=ptr, tables=tables, fragN=fragN, n=len(sizes), S=4, zero_row=zero_row, zero_region=region)
