"""method = "hmp" of getCandidateInteractions (chicdiff.R:2135-2137, 2146) restated for the tests: landau_tail_twin, the numpy
evaluation of the coefficients committed in chicdiff_amd/csrc/landau_table.h (parsed from the header, so there is one copy of
them), operation by operation as devmath.h landau_tail but with a rounded multiply and add where the device has one fused
operation; and candidates_hmp_literal, p.hmp per group on the groups and pairs of candidates_twin.candidates_literal."""
import functools
import json
import math
import os
import re

import numpy as np

import candidates_twin as tw

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HMP_LOC = 0.874367040387922004      # 1 + digamma(1) - log(2 / pi)
HMP_SCALE = math.pi / 2
# The twin's largest error over tests/golden/landau_tail.json in units of 2^-52 Q max(1, (1 + |z|) |d log Q / dz|), measured on the
# CPU by test_landau_tail.py (profiles/r19_landau_accuracy.json, "twin"), and the bound asserted for the twin AND for the device:
# that figure doubled and rounded up to a whole unit.  The factor two is what the device may add by fusing each multiply-add and by
# its own logarithm; it is not taken from the device's figure.
LANDAU_TWIN_MAX_UNITS = 1.064   # at z = 2^1023, where Q is subnormal; 0.461 over the normal range
LANDAU_BOUND_UNITS = 3
_HEX = r"[-+]?0x[0-9a-f.]+p[-+]?\d+"


def load_table(path=os.path.join(ROOT, "chicdiff_amd", "csrc", "landau_table.h")):
    h = open(path).read()
    macro = lambda k: re.search(r"#define CD_LANDAU_%s[ \t]+((?:.*\\\n)*.*)" % k, h).group(1)
    t = {k.lower(): int(macro(k)) for k in ("NUNI", "NOCT", "NINT", "DEG", "NTERMS")}
    t["one"], t["cut"] = float.fromhex(macro("ONE")), float.fromhex(macro("CUT"))
    arr = lambda k: np.array([float.fromhex(x) for x in re.findall(_HEX, macro(k))])
    t["coef"] = arr("COEF_INIT").reshape(t["nint"], t["deg"] + 2)
    t["end"], t["series"] = arr("END_INIT"), arr("SERIES_INIT")
    assert len(t["end"]) == t["nint"] + 1 and len(t["series"]) == t["nterms"] * (t["nterms"] + 1) // 2 + 1
    assert t["nint"] == t["nuni"] + 4 * t["noct"] and t["cut"] == 2.0 ** (t["noct"] + 1)
    return t


def table_bounds(t):
    b = [t["one"] + 0.25 * i for i in range(t["nuni"] + 1)]
    for e in range(1, t["noct"] + 1):
        b += [2.0 ** e * (1 + q / 4) for q in range(1, 5)]
    return np.array(b)


_TABLE = None


def landau_tail_twin(z, t=None):
    global _TABLE
    if t is None:
        t = _TABLE = _TABLE or load_table()
    z = np.atleast_1d(np.asarray(z, dtype=np.float64))
    out = np.full(z.shape, np.nan)
    with np.errstate(all="ignore"):
        out[z <= t["one"]] = 1.0
        far = z > 2.0 ** 100
        out[far] = t["series"][0] / z[far]
        m = (z >= t["cut"]) & ~far
        if m.any():
            zz = z[m]
            L, w = np.log(zz), 1.0 / zz
            acc = np.zeros_like(zz)
            at = len(t["series"])
            for n in range(t["nterms"] - 1, 0, -1):
                at -= n + 1
                pn = np.full_like(zz, t["series"][at + n])
                for j in range(n - 1, -1, -1):
                    pn = pn * L + t["series"][at + j]
                acc = acc * w + pn
            acc = (acc * w + t["series"][1]) + t["series"][0]
            out[m] = np.minimum(acc / zz, t["end"][t["nint"]])
        m = (z > t["one"]) & (z < t["cut"])
        if m.any():
            zz = z[m]
            low = zz < 2.0
            i = np.zeros(zz.shape, dtype=np.int64)
            s = np.zeros_like(zz)
            # below 2: arithmetic on z
            zl = zz[low]
            il = np.minimum(((zl - t["one"]) * 4.0).astype(np.int64), t["nuni"] - 1)
            lo = 0.25 * il + t["one"]
            fix = zl < lo
            il, lo = il - fix, lo - 0.25 * fix
            i[low], s[low] = il, (zl - (lo + 0.125)) * 8.0
            # from 2 on: exponent and two mantissa bits
            b = np.ascontiguousarray(zz[~low]).view(np.uint64)
            i[~low] = t["nuni"] + (b >> np.uint64(50)).astype(np.int64) - 4096
            c = ((b & ~np.uint64((1 << 50) - 1)) | np.uint64(1 << 49)).view(np.float64)
            sc = ((np.uint64(2049) - (b >> np.uint64(52))) << np.uint64(52)).view(np.float64)
            s[~low] = (zz[~low] - c) * sc
            co = t["coef"][i]
            r = co[:, t["deg"] + 1].copy()
            for k in range(t["deg"], 0, -1):
                r = r * s + co[:, k]
            r = r + co[:, 0]
            out[m] = np.minimum(np.maximum(r, t["end"][i + 1]), t["end"][i])
    return out


def hmp_z(ps):
    """z of one group: its p values in pair order -> (x - (log L + c)) / (pi / 2), x the mean of 1 / p' summed sequentially."""
    s = 0.0
    for p in ps:
        pp = 1.0 if (p != p or p > 1.0) else p                        # :2136
        s += (1.0 / pp) if pp != 0.0 else math.copysign(math.inf, pp)
    L = len(ps)
    return (s / L - (math.log(L) + HMP_LOC)) / HMP_SCALE


def candidates_hmp_literal(bait, minOE, maxOE, p, peak_bait, peak_oe, scores, cond1, cond2, merged, score, pvcut, min_delta):
    """candidates_literal's groups and pairs with p.hmp in place of min(): every group's entry [1] is hm_p (the twin's), `z`
    lists the groups' z (groups_all order), `groups` are those the final filter keeps."""
    # pvcut = inf: candidates_literal's own filter then reads only delta; the p filter is redone below on hm_p
    res = tw.candidates_literal(bait, minOE, maxOE, [0.0] * len(p), peak_bait, peak_oe, scores, cond1, cond2, merged, score, math.inf, min_delta)
    z = [hmp_z([p[r] for r in g[3]]) for g in res["groups_all"]]
    hm = landau_tail_twin(np.array(z)) if z else np.zeros(0)
    for g, v in zip(res["groups_all"], hm):
        g[1] = float(v)
    res["z"] = z
    res["groups"] = [g for g in res["groups_all"] if g[1] <= pvcut and g[2] == g[2] and g[2] >= min_delta]
    res["z_kept"] = [zz for g, zz in zip(res["groups_all"], z) if g[1] <= pvcut and g[2] == g[2] and g[2] >= min_delta]
    return res


def fmt_replaced(x):
    """as.character() of a pcol value after :2136."""
    return tw.fmt_double(1.0 if (x != x or x > 1.0) else x)


@functools.lru_cache(maxsize=None)
def golden():
    """(z, Q, unit) as float64 arrays plus the exact strings: shared, read once."""
    g = json.load(open(os.path.join(ROOT, "tests", "golden", "landau_tail.json")))
    z = np.array([math.inf if x == "inf" else float.fromhex(x) for x in g["z"]])
    return g, z


def error_units(z, got, g):
    """|got - Q| / u(z) per abscissa, in 40-digit arithmetic; where u = 0 (z = inf) 0 for an exact hit, inf otherwise."""
    import mpmath as mp
    out = np.zeros(len(z))
    with mp.workdps(40):
        for k, (zi, v, Q, D) in enumerate(zip(z, got, g["Q"], g["dlogQ_dz"])):
            Q, D = mp.mpf(Q), mp.mpf(D)
            e = abs(mp.mpf(float(v)) - Q)
            if zi == math.inf or Q == 0:
                out[k] = 0.0 if e == 0 else math.inf
            else:
                out[k] = float(e / (mp.mpf(2) ** -52 * Q * max(1, (1 + abs(mp.mpf(float(zi)))) * abs(D))))
    return out


def record(key, worst, at):
    out = os.environ.get("CHICDIFF_ACCURACY_OUT")   # a directory: keep the measured figure (-> profiles/r19_landau_accuracy.json)
    if not out:
        return
    os.makedirs(out, exist_ok=True)
    path = os.path.join(out, "r19_landau_accuracy.json")
    doc = json.load(open(path)) if os.path.exists(path) else {}
    doc.update(unit="2^-52 * Q(z) * max(1, (1 + |z|) * |d log Q / dz|)", bound_asserted=LANDAU_BOUND_UNITS)
    doc[key] = dict(max_units=worst, at_z=float.hex(at), abscissae=len(golden()[1]))
    with open(path, "w") as f:
        json.dump(doc, f, indent=1)


def unit_at(z):
    """u(z) = 2^-52 Q max(1, (1 + |z|) |d log Q / dz|) from the twin itself (a central difference is enough for a scale)."""
    z = np.atleast_1d(np.asarray(z, dtype=np.float64))
    with np.errstate(all="ignore"):
        h = 1e-4 * np.maximum(1.0, np.abs(z))
        q = landau_tail_twin(z)
        d = (np.log(landau_tail_twin(z + h)) - np.log(landau_tail_twin(z - h))) / (2 * h)
        cond = np.where(np.isfinite(d), (1 + np.abs(z)) * np.abs(d), 1.0)
        return 2.0 ** -52 * q * np.maximum(1.0, cond)


def candidates_table_hmp_literal(output, peaks, cond1names, cond2names, merged, score, pcol, pvcut, min_delta):
    """:2135-2161 for method = "hmp": candidates_twin.candidates_table_literal's table with hm_<pcol> in place of min_<pcol> and the
    pasted <pcol> column showing the values AFTER :2136 (NA and > 1 print as 1).  Returns (rows, z of each row's group)."""
    names = list(cond1names) + list(cond2names)
    scores = [[peaks[c][i] for c in names] for i in range(len(peaks["baitID"]))]
    c1, c2 = list(range(len(cond1names))), list(range(len(cond1names), len(names)))
    res = candidates_hmp_literal(output["baitID"], output["minOE"], output["maxOE"], output[pcol], peaks["baitID"], peaks["oeID"], scores,
                                 c1, c2, merged, score, pvcut, min_delta)
    rows = []
    for i, hm, d, rs in res["groups"]:
        row = {"baitID": peaks["baitID"][i], "oeID": peaks["oeID"][i], "baitChr": peaks["baitChr"][i],
               "baitstart": output["baitstart"][rs[0]], "baitend": output["baitend"][rs[0]], "baitName": peaks["baitName"][i]}
        for c in names:
            row[c] = peaks[c][i]
        row["hm_" + pcol] = hm
        row["deltaAsinhScore"] = d
        row["regionIDs"] = ",".join(str(output["regionID"][r]) for r in rs)
        row["log2FoldChanges"] = ",".join(tw.fmt_double(output["log2FoldChange"][r]) for r in rs)
        row[pcol] = ",".join(fmt_replaced(output[pcol][r]) for r in rs)
        row["OEranges"] = ",".join(f"{output['OEstart'][r]}-{output['OEend'][r]}" for r in rs)
        rows.append(row)
    return rows, res["z_kept"]
