"""The normalisation stage under a 50-digit judge: Bmean / Tmean / FullMean per fragment pair (a3), the sums by region (a2), the size
factors (a5) and the offsets with the theta mix (a4), on the small cases of tests/norm_inputs.py.

Until here these steps were held to the project's own CPU oracle at rtol = 1e-13 on one benign input each, and both sides of each of
those comparisons were written by one hand from one reading of chicdiff.R.  tests/norm_twin.py shares no code with either and was
written from the reference's lines alone; this module puts

  * the CPU oracle under it: every exact requirement (N sums; the NaN / Inf places of Bmean, Tmean, FullMean and of the region sums;
    which rows take the size factors; Tmean bit for bit) on EVERY element, and per stratum (quantity x row class) the worst error in
    the units of norm_twin.py within the bound its docstring derives by counting roundings;
  * fifteen wrong readings of the reference, each applied to a plain numpy restatement, under the same judge: each must be rejected
    on the planted inputs while the right formulas pass;
  * the host's chicEstimateDistFunValues against an exact least-squares fit.

tests/test_gpu_norm.py runs the same cases and the same judge over the kernels, with the oracle of this module as the yardstick."""
import math
from collections import defaultdict

import mpmath as mp
import numpy as np
import pytest

import norm_inputs as ni
import norm_twin as nt


@pytest.fixture(scope="module")
def oracle():
    import __graft_entry__ as g
    g.build()
    from oracle import oracle as o
    return o


# ---------------------------------------------------------------------------------------------------------------------------
# the judge
# ---------------------------------------------------------------------------------------------------------------------------
def same_bits(a, b):
    a, b = np.ascontiguousarray(a, dtype=np.float64), np.ascontiguousarray(b, dtype=np.float64)
    return (a.view(np.int64) == b.view(np.int64)) | (np.isnan(a) & np.isnan(b))


class Verdict:
    """errors: stratum (quantity, class) -> list of errors in units; violations: exact requirements that do not hold"""

    def __init__(self):
        self.errors = defaultdict(list)
        self.violations = []

    def value(self, stratum, where, got, exact, unit):
        """one element: an exact requirement where the twin's value is a float (NaN / Inf / a copy) or its unit is 0"""
        got = float(got)
        if nt.special(exact):
            ok = math.isnan(got) if math.isnan(exact) else got == exact
            if not ok:
                self.violations.append((stratum, where, got, exact))
            return
        if not math.isfinite(got):
            self.violations.append((stratum, where, got, float(exact)))
        elif unit == 0:
            if mp.mpf(got) != exact:
                self.violations.append((stratum, where, got, float(exact)))
            else:
                self.errors[stratum].append(0.0)
        else:
            self.errors[stratum].append(float(abs(mp.mpf(got) - exact) / unit))

    def worst(self):
        return {k: (max(v), len(v)) for k, v in self.errors.items()}

    def merge(self, other):
        for k, v in other.errors.items():
            self.errors[k] += v
        self.violations += other.violations
        return self


def rejected(verdict, bound):
    """bound: stratum -> units"""
    return bool(verdict.violations) or any(w > bound(k) for k, (w, _) in verdict.worst().items())


_TWIN = {}


def twin_of(key, make):
    if key not in _TWIN:
        _TWIN[key] = make()
    return _TWIN[key]


def judge_a3(key, case, B, Tm, F):
    """B, Tm, F: (S, nru) doubles; any of them may be None (not asked for)"""
    ref = twin_of(("a3", key), lambda: nt.fragment_background(**case["args"]))
    v = Verdict()
    S, nru = len(ref["B"]), len(case["rows"])
    with mp.workdps(nt.DPS):
        for s in range(S):
            if Tm is not None:
                bad = np.flatnonzero(~same_bits(Tm[s], np.array(ref["T"][s])))
                v.violations += [(("Tmean", "bits"), (s, int(r)), float(Tm[s][r]), ref["T"][s][r]) for r in bad]
            for r in range(nru):
                cls = ref["cls"][s][r]
                if B is not None:
                    v.value(("Bmean", cls), (s, r), B[s][r], ref["B"][s][r], ref["uB"][s][r])
                if F is not None:
                    v.value(("FullMean", cls), (s, r), F[s][r], ref["F"][s][r], ref["uF"][s][r])
    return v


def a3_bound(stratum):
    return nt.BOUND_LOGB if stratum[0] == "Bmean" else nt.BOUND_FULLMEAN


def judge_a2(key, case, N, FM, ref=None):
    """N, FM: (n, S); either may be None"""
    if ref is None:
        ref = twin_of(("a2", key), lambda: nt.window_sums(case["fragN"], case["fragFM"], case["region_ptr"]))
    rN, rF, uF = ref
    v = Verdict()
    sizes = np.diff(case["region_ptr"])
    blocks = set(case.get("direct_blocks", ()))
    with mp.workdps(nt.DPS):
        if N is not None:
            want = np.array(rN, dtype=np.int64).reshape(len(sizes), -1)
            bad = np.argwhere(np.asarray(N, dtype=np.int64) != want)
            v.violations += [(("N", "sum"), tuple(int(x) for x in ij), int(N[tuple(ij)]), int(want[tuple(ij)])) for ij in bad]
        if FM is not None:
            for i in range(len(sizes)):
                cls = ("direct path, " if i // 256 in blocks else "staged, ") + ("F <= 1" if sizes[i] <= 1 else "F <= 13" if sizes[i] <= 13 else "F = 4000")
                for j in range(len(rF[i])):
                    v.value(("region sum", cls), (i, j), FM[i][j], rF[i][j], uF[i][j])
    return v


def judge_a5(key, counts, sf):
    ref = twin_of(("a5", key), lambda: nt.size_factors(counts))
    v = Verdict()
    S = counts.shape[1]
    with mp.workdps(nt.DPS):
        for j in range(S):
            v.value(("size factor", f"S = {S}"), (key, j), sf[j], ref[0][j], ref[1][j])
    return v


def offsets_class(S, theta, na):
    return ("class kernel (S <= 16)" if S <= 16 else "generic kernel (S > 16)") + (", unmixed" if theta is None else ", mixed") + (", NA row" if na else "")


def judge_a4(key, fm, sf, theta, out):
    """out: (n, S).  Unmixed rows that take the size factors must BE them (bits); everything else in units."""
    make = lambda: nt.offsets(fm, sf, theta)
    ref, unit, na = twin_of(("a4", key, theta), make) if key is not None else make()
    v = Verdict()
    n, S = fm.shape
    with mp.workdps(nt.DPS):
        for i in range(n):
            st = ("offsets", offsets_class(S, theta, na[i]))
            for j in range(S):
                v.value(st, (i, j), out[i][j], ref[i][j], unit[i][j])
    return v, na


def a4_bound(S, theta):
    return lambda stratum: nt.bound_offsets(S, theta is not None)


# ---------------------------------------------------------------------------------------------------------------------------
# engines: the CPU oracle behind the calls the judge knows (tests/test_gpu_norm.py has the device's)
# ---------------------------------------------------------------------------------------------------------------------------
class OracleEngine:
    def __init__(self, o):
        self.o = o

    def background(self, args):
        """The oracle takes a row off the map for a caller's error (RuntimeError) where the library gives NA (include/chicdiff_hip.h; the
        reference's merge with all.x = TRUE leaves NA there): it is given the rows on the map, the others stay NaN."""
        b, o = args["bait"].astype(np.int64) - args["id_min"], args["oe"].astype(np.int64) - args["id_min"]
        nid = len(args["midsum"])
        on = (b >= 0) & (b < nid) & (o >= 0) & (o < nid)
        if not on.all():
            with pytest.raises(RuntimeError):
                self.o.fragment_background(**args)
        outs = [np.full((args["sj"].shape[0], len(b)), np.nan) for _ in range(3)]
        for full, part in zip(outs, self.o.fragment_background(**dict(args, bait=args["bait"][on], oe=args["oe"][on]))):
            full[:, on] = part
        return outs

    def sums(self, fn, fm, ptr):
        N, FM = self.o.window_sums(fn, fm, ptr)
        return (N if fn is not None else None), (FM if fm is not None else None)

    def size_factors(self, counts):
        return self.o.size_factors(counts)

    def offsets(self, fm, sf, theta):
        return self.o.offsets(fm, sf, theta)


A2_MODES = ["both", "fragN alone", "fragFM alone"]


def run_a2(engine, name, mode):
    case = ni.a2_case(name)
    fn = case["fragN"] if mode != "fragFM alone" else None
    fm = case["fragFM"] if mode != "fragN alone" else None
    N, FM = engine.sums(fn, fm, case["region_ptr"])
    assert (N is None) == (fn is None) and (FM is None) == (fm is None)
    return case, judge_a2(name, case, N, FM)


def run_chain(engine, ch):
    """a3 -> a2 -> a5 -> a4 on the chained case, each stage judged on the doubles and ints it was really given.  Returns the verdicts
    and the values."""
    a = ch["a3"]
    B, Tm, F = engine.background(a["args"])
    v3 = judge_a3("chain", a, B, Tm, F)
    fragFM = np.ascontiguousarray(np.asarray(F).T)
    N, FM = engine.sums(ch["fragN"], fragFM, ch["region_ptr"])
    sums_case = dict(fragN=ch["fragN"], fragFM=fragFM, region_ptr=ch["region_ptr"])
    v2 = judge_a2(None, sums_case, N, FM, ref=nt.window_sums(ch["fragN"], fragFM, ch["region_ptr"]))
    N, FM = np.asarray(N), np.asarray(FM)
    sf = engine.size_factors(N)
    v5 = judge_a5(("chain", N.tobytes()), N, sf)
    out = {}
    v4 = Verdict()
    nas = None
    for theta in (None, 0.5):
        out[theta] = np.asarray(engine.offsets(FM, sf, theta))
        v, nas = judge_a4(None, FM, sf, theta, out[theta])
        v4.merge(v)
    return dict(a3=v3, a2=v2, a5=v5, a4=v4), dict(F=np.asarray(F), N=N, FM=FM, sf=np.asarray(sf), out=out, na=nas)


def check_chain_facts(ch, val):
    r, g = ch["zero_row"], ch["zero_region"]
    assert np.all(np.isposinf(val["F"][:, r])), "dist = 0: FullMean is +Inf"
    assert np.all(np.isposinf(val["FM"][g])), "its region's sum is +Inf"
    assert val["na"][g] and np.array_equal(val["out"][None][g], val["sf"]), "and the region's offsets are the size factors"
    assert any(val["na"][i] and np.isnan(val["FM"][i]).any() for i in range(ch["n"])) and not all(val["na"])


# ---------------------------------------------------------------------------------------------------------------------------
# the inputs are what they are called
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("S", ni.A3_S)
def test_a3_planted_rows_are_present(S):
    case = ni.a3_case(S)
    ref = twin_of(("a3", S), lambda: nt.fragment_background(**case["args"]))
    p, a = case["planted"], case["args"]
    assert len(case["rows"]) <= 3000 and all(len(v) > 0 for v in p.values())
    cls = ref["cls"][0]
    heads = [ref["dist"][r] for r in p["neighbours"] if cls[r] == "head"]
    assert min(heads) < 0 < max(heads) and len(heads) >= 4 and all(cls[r] == "tail" for r in p["far"])
    assert all(cls[r] == "dist 0" and ref["dist"][r] == 0 for r in p["dist 0"]) and all(cls[r] == "off map" for r in p["off map"])
    assert all(ref["B"][0][r] == math.inf and ref["F"][0][r] == math.inf for r in p["dist 0"])
    ids = {(int(a["bait"][r]), int(a["oe"][r])) for r in p["map ends"]}
    assert any(o == a["id_min"] for _, o in ids) and any(o == a["id_min"] + len(a["midsum"]) - 1 for _, o in ids)
    d2 = lambda r: int(a["midsum"][case["rows"][r][1]]) - int(a["midsum"][case["rows"][r][0]])
    for name, sign, up in (("odd down +", 1, 0), ("odd up +", 1, 1), ("odd down -", -1, 0), ("odd up -", -1, 1)):
        for r in p[name]:
            assert d2(r) % 2 == 1 and d2(r) * sign > 0 and ref["dist"][r] == (d2(r) + (1 if up else -1)) // 2 and ref["dist"][r] % 2 == 0
    for r in p["midpoints rounded apart"]:
        b, o = case["rows"][r]
        assert np.rint(a["midsum"][o] / 2.0) - np.rint(a["midsum"][b] / 2.0) != ref["dist"][r]
    # ld at obs.min / obs.max: the double log of the edge row's distance is obs.min / obs.max itself or its neighbour, both sides
    (rlo,), (rhi,) = p["at obs.min"], p["at obs.max"]
    for s in range(S):
        for r, k, l in ((rlo, 8, case["lmin"]), (rhi, 9, case["lmax"])):
            assert l == np.log(float(abs(ref["dist"][r]))) and abs(a["distfun"][s][k] - l) <= np.spacing(l)
    kinds = {(case["edge"][s], ref["cls"][s][rlo], ref["cls"][s][rhi]) for s in range(S)}
    if S >= 4:
        assert len({k[0] for k in kinds}) == 3 and {"head", "cubic"} <= {k[1] for k in kinds} and {"tail", "cubic"} <= {k[2] for k in kinds}
    nan = math.isnan
    for s in range(S):
        (r,) = p["tlb missing, tblb partly NaN"]
        row = a["T"][s][2]
        assert ref["T"][s][r] == np.nanmin(row) and np.isnan(row).any() and np.nanmin(row) > np.nanmin(a["T"][s])
        assert nan(ref["T"][s][p["tlb missing, tblb all NaN"][0]]) and nan(ref["T"][s][p["cell NaN"][0]])
        assert all(not nan(ref["T"][s][r]) for r in p["cell seen"][:1])
        assert all(nan(ref["B"][s][r]) and nan(ref["F"][s][r]) for r in p["s_j NaN, tblb set"]) and not nan(ref["T"][s][p["s_j NaN, tblb set"][0]])
        assert all(not nan(float(ref["B"][s][r])) for r in p["s_i NaN"]) and all(nan(a["si"][s][case["rows"][r][1]]) for r in p["s_i NaN"])
    finite = [float(x) for s in range(S) for x in ref["F"][s] if not nt.special(x)]
    assert finite and 1e-250 < min(finite) and max(finite) < 1e250   # no FullMean near overflow or underflow


def test_a2_planted_regions_are_present():
    c = ni.a2_case("blocks")
    assert c["n"] <= 650 and c["direct_blocks"] == [1] and c["nblocks"] == 3   # a direct-path block between two staged ones
    s = c["sizes"]
    assert s[0] == 0 and s[-1] == 0 and s[:3] == [0, 0, 0] and set(range(1, 12)) <= set(s) and s.count(13) == 300
    long = ni.a2_case("one long region")
    assert 4000 in long["sizes"] and long["direct_blocks"] == [0] and long["nblocks"] == 2
    assert [ni.a2_case(k)["n"] for k in ("n1", "n255", "n256", "n257")] == [1, 255, 256, 257]
    for name in ("blocks", "one long region", "n255", "n256", "n257"):
        c = ni.a2_case(name)
        fm, ptr, p = c["fragFM"], c["region_ptr"], c["planted"]
        seg = lambda r: fm[ptr[r]:ptr[r + 1]]
        assert np.isnan(seg(p["nan"][0])).any() and np.isposinf(seg(p["inf"][0])).any() and not np.isnan(seg(p["inf"][0])).any()
        assert np.isnan(seg(p["inf_and_nan"][0])).any() and np.isposinf(seg(p["inf_and_nan"][0])).any()
        for r in p["wide"]:
            assert seg(r).max(axis=0).min() / seg(r).min(axis=0).max() > 1e11
        assert nt.far_from_overflow(fm)


def test_a4_planted_rows_are_present():
    assert sorted({S for S, _ in ni.A4_SHAPES}) == [2, 3, 4, 5, 8, 9, 12, 16, 17, 20] and {n for _, n in ni.A4_SHAPES} == {1, 255, 257, 1030}
    assert ni.THETAS == [None, 0.0, 0.25, 0.5, 1.0]
    for S, n in ni.A4_SHAPES:
        c = ni.a4_case(S, n)
        assert nt.far_from_overflow(c["fm"]) and abs(np.log(c["sf"]).mean()) > 1e-3
        na = [nt.row_is_na(r) for r in c["fm"]]
        assert sum(na) == sum(len(v) for k, v in c["planted"].items() if k not in ("equal values", "wide"))
        if n > 1:
            assert len(c["planted"]) == 10 and na[0] and na[n - 1] and not na[10]
            assert c["fm"][11:21].max() / c["fm"][11:21].min() >= 1e59 and len(set(c["fm"][10])) == 1


@pytest.fixture(scope="module")
def hiplib():
    import test_size_factors_direct as sfd
    import __graft_entry__ as g
    g.build()
    from chicdiff_amd import hip
    return hip.load_library(), sfd


def test_a5_planted_matrices_meet_the_select_paths(hiplib):
    """the two-bin split and a list longer than kSfCand are really met (the numpy restatement of the direct select on the library's own bins)"""
    L, sfd = hiplib
    cases = ni.a5_cases()
    assert {v.shape[1] for v in cases.values()} >= {1, 2, 4, 5, 8, 9, 16}
    used = {k: int((v > 0).all(axis=1).sum()) for k, v in cases.items()}
    assert used["one used row"] == 1 and used["two used rows"] == 2 and used["odd 1001x5"] % 2 == 1 and used["even 1000x9"] % 2 == 0
    assert cases["up to 2^31-1"].max() == 2 ** 31 - 1 and (cases["zeros_and_negatives"] == ni.NA_INT).any() and (cases["zeros_and_negatives"] == -1).any()
    _, seen = sfd.direct_medians(L, cases["split_middles"])
    assert seen["split"] == 2
    _, seen = sfd.direct_medians(L, cases["ties 3001x4"])
    assert seen["fallback"] > 0 and seen["longest_list"] > sfd.CAND
    keys = sfd.keys_of(cases["column_x1000000"])
    assert keys[:, 2].min() > sfd.LO + sfd.SPAN                       # beyond the binned range
    _, seen = sfd.direct_medians(L, cases["column_x1000000"])
    assert seen["fallback"] > 0


# ---------------------------------------------------------------------------------------------------------------------------
# the oracle under the judge
# ---------------------------------------------------------------------------------------------------------------------------
def report(tag, verdict, bound):
    for k, (w, n) in sorted(verdict.worst().items()):
        print(f"{tag} | {k[0]} | {k[1]}: n={n} worst {w:.3f} units, bound {bound(k):g}")


@pytest.mark.parametrize("S", ni.A3_S)
def test_oracle_fragment_background(oracle, S):
    case = ni.a3_case(S)
    B, Tm, F = OracleEngine(oracle).background(case["args"])
    v = judge_a3(S, case, B, Tm, F)
    report(f"a3 S={S}", v, a3_bound)
    assert not v.violations, v.violations[:10]
    assert not rejected(v, a3_bound), v.worst()


@pytest.mark.parametrize("mode", A2_MODES)
@pytest.mark.parametrize("name", ni.A2_CASES)
def test_oracle_window_sums(oracle, name, mode):
    case, v = run_a2(OracleEngine(oracle), name, mode)
    report(f"a2 {name} {mode}", v, lambda k: nt.BOUND_SUM)
    assert not v.violations, v.violations[:10]
    assert not rejected(v, lambda k: nt.BOUND_SUM), v.worst()


def test_oracle_size_factors(oracle):
    for name, counts in ni.a5_cases().items():
        v = judge_a5(name, counts, oracle.size_factors(counts))
        S = counts.shape[1]
        report(f"a5 {name}", v, lambda k: nt.bound_sf(S))
        assert not v.violations, (name, v.violations)
        assert not rejected(v, lambda k: nt.bound_sf(S)), (name, v.worst())


@pytest.mark.parametrize("S,n", ni.A4_SHAPES)
def test_oracle_offsets(oracle, S, n):
    case = ni.a4_case(S, n)
    for theta in ni.THETAS:
        out = oracle.offsets(case["fm"], case["sf"], theta)
        v, na = judge_a4((S, n), case["fm"], case["sf"], theta, out)
        report(f"a4 S={S} n={n} theta={theta}", v, a4_bound(S, theta))
        assert not v.violations, (theta, v.violations[:10])
        assert not rejected(v, a4_bound(S, theta)), (theta, v.worst())
        assert na == [nt.row_is_na(r) for r in case["fm"]]


def test_standard_norm_is_the_size_factors():
    case = ni.a4_case(5, 1)
    out, unit, na = nt.offsets(case["fm"], case["sf"], None, norm="standard")
    assert out == [list(case["sf"])] and not any(na)


def test_oracle_chain(oracle):
    ch = ni.chained_case()
    verdicts, val = run_chain(OracleEngine(oracle), ch)
    bounds = dict(a3=a3_bound, a2=lambda k: nt.BOUND_SUM, a5=lambda k: nt.bound_sf(4), a4=lambda k: nt.bound_offsets(4, "mixed" in k[1] and "unmixed" not in k[1]))
    for stage, v in verdicts.items():
        report(f"chain {stage}", v, bounds[stage])
        assert not v.violations, (stage, v.violations[:10])
        assert not rejected(v, bounds[stage]), (stage, v.worst())
    check_chain_facts(ch, val)


# ---------------------------------------------------------------------------------------------------------------------------
# wrong readings of the reference, on a plain numpy restatement
# ---------------------------------------------------------------------------------------------------------------------------
def np_background(args, wrong=None):
    a = args
    nid, S = len(a["midsum"]), a["sj"].shape[0]
    b, o = a["bait"].astype(np.int64) - a["id_min"], a["oe"].astype(np.int64) - a["id_min"]
    on = (b >= 0) & (b < nid) & (o >= 0) & (o < nid)
    bc, oc = np.where(on, b, 0), np.where(on, o, 0)
    half = (a["midsum"][oc] - a["midsum"][bc]) / 2.0
    dist = np.rint(half)
    if wrong == "round half away from zero":
        dist = np.sign(half) * np.floor(np.abs(half) + 0.5)
    if wrong == "midpoints rounded separately":
        dist = np.rint(a["midsum"][oc] / 2.0) - np.rint(a["midsum"][bc] / 2.0)
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        ld = np.log(np.abs(dist))
        B, Tm = np.full((S, len(b)), np.nan), np.full((S, len(b)), np.nan)
        for s in range(S):
            p = a["distfun"][s]
            cubic = p[0] + p[1] * ld + p[2] * ld ** 2 + p[3] * ld ** 3
            head, tail = p[4] + ld * p[5], p[6] + ld * p[7]
            if wrong == "head and tail lines exchanged":
                head, tail = tail, head
            e = np.where(ld > p[9], tail, np.where(ld < p[8], head, cubic))
            if wrong == "cubic outside the observed range":
                e = cubic
            si = a["si"][s, oc]
            if wrong != "s_i NA left NA":
                si = np.where(np.isnan(si), 1.0, si)
            B[s] = np.where(on, a["sj"][s, bc] * si * np.exp(e), np.nan)
            tb, tl = a["tblb"][s, bc], a["tlb"][s, oc]
            T = a["T"][s]
            both, only = on & (tb >= 0) & (tl >= 0), on & (tb >= 0) & (tl < 0)
            Tm[s, both] = T[tb[both], tl[both]]
            if wrong == "missing tlb -> NA":
                pass
            elif wrong == "minimum over the whole Tmean table":
                Tm[s, only] = np.nanmin(T)
            else:
                low = np.array([np.min(r[~np.isnan(r)]) if (~np.isnan(r)).any() else np.nan for r in T])
                Tm[s, only] = low[tb[only]]
        return B, Tm, B + Tm


def np_sums(fn, fm, ptr, wrong=None):
    n = len(ptr) - 1
    add = np.nansum if wrong == "region sum with na.rm" else np.sum
    N = np.array([fn[ptr[i]:ptr[i + 1]].sum(axis=0) for i in range(n)])
    FM = np.array([add(fm[ptr[i]:ptr[i + 1]], axis=0) for i in range(n)])
    return N, FM


def np_size_factors(counts, wrong=None):
    k = counts.astype(np.float64)
    with np.errstate(divide="ignore", invalid="ignore"):
        l = np.where(k > 0, np.log(k), np.nan)
    S = k.shape[1]
    if wrong == "rows with a zero kept, with their positive counts":
        keys = l - np.nanmean(np.where(np.isnan(l).all(axis=1, keepdims=True), 0.0, l), axis=1, keepdims=True)
        cols = [keys[~np.isnan(keys[:, j]), j] for j in range(S)]
    else:
        use = (counts > 0).all(axis=1)
        keys = l[use] - l[use].sum(axis=1, keepdims=True) / S
        cols = [keys[:, j] for j in range(S)]
    med = []
    for c in cols:
        c = np.sort(c)
        m = len(c)
        med.append(c[(m - 1) // 2] if wrong == "lower middle of an even count" else np.median(c))
    sf = np.exp(np.array(med))
    if wrong == "size factors renormalised to geometric mean 1":
        sf = sf / np.exp(np.log(sf).mean())
    return sf


def np_offsets(fm, sf, theta, wrong=None):
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        m3 = fm / np.exp(np.log(fm).mean(axis=1, keepdims=True))
        na = np.isnan(m3).any(axis=1)
        if wrong == "NA row -> 1":
            m3[na] = 1.0
        elif wrong == "only the NA cells replaced":
            m3 = np.where(np.isnan(m3), sf[None, :], m3)
        else:
            m3[na] = sf
        if theta is None:
            return m3
        if wrong == "geometric mix (:1636)":
            sc = np.exp(np.log(m3) * (1 - theta) + np.log(sf)[None, :] * theta)
        else:
            sc = m3 * (1 - theta) + sf[None, :] * theta
        if wrong == "mix without the second renormalisation":
            return sc
        return sc / np.exp(np.log(sc).mean(axis=1, keepdims=True))


A3_WRONG = ["round half away from zero", "midpoints rounded separately", "s_i NA left NA", "missing tlb -> NA", "minimum over the whole Tmean table",
            "cubic outside the observed range", "head and tail lines exchanged"]
A2_WRONG = ["region sum with na.rm"]
A5_WRONG = ["lower middle of an even count", "rows with a zero kept, with their positive counts", "size factors renormalised to geometric mean 1"]
A4_WRONG = ["NA row -> 1", "only the NA cells replaced", "mix without the second renormalisation", "geometric mix (:1636)"]


@pytest.mark.parametrize("wrong", [None] + A3_WRONG)
def test_judge_rejects_wrong_background(wrong):
    case = ni.a3_case(4)
    v = judge_a3(4, case, *np_background(case["args"], wrong))
    report(f"a3 variant {wrong}", v, a3_bound)
    assert rejected(v, a3_bound) == (wrong is not None), (wrong, v.violations[:5], v.worst())


@pytest.mark.parametrize("wrong", [None] + A2_WRONG)
def test_judge_rejects_wrong_sums(wrong):
    case = ni.a2_case("n256")
    v = judge_a2("n256", case, *np_sums(case["fragN"], case["fragFM"], case["region_ptr"], wrong))
    assert rejected(v, lambda k: nt.BOUND_SUM) == (wrong is not None), (wrong, v.violations[:5], v.worst())


@pytest.mark.parametrize("wrong", [None] + A5_WRONG)
def test_judge_rejects_wrong_size_factors(wrong):
    """the right formulas pass on every matrix; a wrong one is rejected on at least one (a lower middle cannot show on an odd count)"""
    hit = []
    for name, counts in ni.a5_cases().items():
        S = counts.shape[1]
        if rejected(judge_a5(name, counts, np_size_factors(counts, wrong)), lambda k: nt.bound_sf(S)):
            hit.append(name)
    print(wrong, "rejected on", hit)
    assert bool(hit) == (wrong is not None), (wrong, hit)
    if wrong == "lower middle of an even count":
        assert {"two used rows", "even 1000x9", "split_middles"} <= set(hit) and "odd 1001x5" not in hit


@pytest.mark.parametrize("wrong", [None] + A4_WRONG)
def test_judge_rejects_wrong_offsets(wrong):
    hit = []
    for S, n in [(4, 257), (17, 1030)]:
        case = ni.a4_case(S, n)
        for theta in ni.THETAS:
            v, _ = judge_a4((S, n), case["fm"], case["sf"], theta, np_offsets(case["fm"], case["sf"], theta, wrong))
            if rejected(v, a4_bound(S, theta)):
                hit.append((S, theta))
    print(wrong, "rejected at", hit)
    assert bool(hit) == (wrong is not None), (wrong, hit)
    if wrong in ("NA row -> 1", "only the NA cells replaced"):
        assert (4, None) in hit and (17, None) in hit
    if wrong == "geometric mix (:1636)":
        assert {(4, 0.25), (4, 0.5), (17, 0.25), (17, 0.5)} <= set(hit)


# ---------------------------------------------------------------------------------------------------------------------------
# chicEstimateDistFunValues (host)
# ---------------------------------------------------------------------------------------------------------------------------
def distfun_bound(nbins):
    """Units the host fit may reach: its solver is backward stable — the computed coefficients are the exact ones of a design matrix
    and data perturbed by at most gamma = c n p u relative to their columns' norms (Higham, Accuracy and Stability of Numerical
    Algorithms, 2nd ed., Theorem 20.3 for Householder QR; LAPACK's SVD-based driver has a bound of the same form) — with n bins, p = 4
    columns and c = 8 for the constant those theorems leave open; before that each element of the design matrix carries 3 roundings
    (log, square, cube), the data 1, and the evaluation of the curve its own 7 (norm_twin.py, log Bmean)."""
    return 8.0 * nbins * 4 + 3 + 1 + 7


DISTFUN_BINS = [10, 40, 75]


def distfun_worst(nbins):
    """worst error, in units, of the host's fitted curve at the bins' midpoints and on the head and tail lines"""
    from chicdiff_amd import pipeline
    rng = np.random.default_rng(nbins)
    mid = 10000.0 + 20000.0 * np.arange(nbins)
    values = np.exp(14.0 - 1.6 * np.log(mid) + 0.05 * np.log(mid) ** 2 - 0.003 * np.log(mid) ** 3 + rng.normal(0, 0.05, nbins))
    values = np.sort(values)[::-1].copy()
    p = pipeline.chicEstimateDistFunValues(values)
    ref = nt.distfun_fit(values)
    with mp.workdps(2 * nt.DPS):
        assert p[8] == float(ref["params"][8]) and p[9] == float(ref["params"][9])   # correctly rounded logs of the end midpoints
        q = [mp.mpf(float(v)) for v in p]
        worst = 0.0
        at = list(ref["x"]) + [mp.log(300), mp.log(5000), ref["x"][-1] + 1, ref["x"][-1] + 3]   # the bins' midpoints, the head and the tail lines
        for ld in at:
            val, cond = ref["curve"](ld)
            if ld > q[9]:
                got = q[6] + q[7] * ld
            elif ld < q[8]:
                got = q[4] + q[5] * ld
            else:
                got = q[0] + q[1] * ld + q[2] * ld ** 2 + q[3] * ld ** 3
            worst = max(worst, float(abs(got - val) / (nt.U * cond)))
    return worst


@pytest.mark.parametrize("nbins", DISTFUN_BINS)
def test_distfun_values_against_exact_least_squares(nbins):
    worst = distfun_worst(nbins)
    print(f"chicEstimateDistFunValues, {nbins} bins: worst error of the fitted curve {worst:.3f} units, bound {distfun_bound(nbins):g}")
    assert worst <= distfun_bound(nbins)


def test_exact_fit_returns_a_line_it_was_given():
    """the judge's own fit: data on a line in log-log come back as that line, with the head and the tail continuing it"""
    mid = 10000.0 + 20000.0 * np.arange(40)
    exact = nt.distfun_fit(np.exp(2.0 - 0.5 * np.log(mid)))
    p = exact["params"]
    assert abs(p[1] + 0.5) < 1e-9 and abs(p[2]) < 1e-9 and abs(p[3]) < 1e-9 and abs(p[5] + 0.5) < 1e-9 and abs(p[7] + 0.5) < 1e-9
    assert abs(exact["curve"](mp.log(300))[0] - (2.0 - 0.5 * mp.log(300))) < 1e-9
