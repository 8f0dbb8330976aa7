#!/usr/bin/env python3
"""Write tests/golden/landau_tail.json: Q(z), the Landau tail of harmonicmeanp::p.hmp, and d log Q / dz as 25-digit strings at
about 2 000 abscissae (hex doubles), from tools/landau_ref.py at 50 digits (60 below zero, where 1 - Q is computed directly from
Zolotarev's form: the Laplace form's integrand cancels there).  Data only.  The abscissae: a grid on [-14, 40]; every interval
bound of chicdiff_amd/csrc/landau_table.h, the cut-over to the expansion among them, and its two neighbouring doubles; powers of
two up to 2^1023; +inf.  Also the four rows of Table 1 of Wilson 2019 (PNAS 116:1195) that the formula must reproduce: the
published alpha = 0.05 thresholds map back to 0.05 within their two-digit rounding.  Run by hand from the repository root."""
import json
import math
import multiprocessing as mpc
import os
import re
import sys

import mpmath as mp

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import landau_ref as lr  # noqa: E402


def table_bounds():
    h = open(os.path.join(ROOT, "chicdiff_amd", "csrc", "landau_table.h")).read()
    d = lambda k: re.search(r"#define CD_LANDAU_%s (\S+)" % k, h).group(1)
    one, nuni, noct = float.fromhex(d("ONE")), int(d("NUNI")), int(d("NOCT"))
    b = [one + 0.25 * i for i in range(nuni + 1)]
    for e in range(1, noct + 1):
        b += [2.0 ** e * (1 + q / 4) for q in range(1, 5)]
    assert b[-1] == float.fromhex(d("CUT"))
    return b


def abscissae():
    zs = [-14.0 + 54.0 * k / 1399 for k in range(1400)]
    for b in table_bounds():
        zs += [math.nextafter(b, -math.inf), b, math.nextafter(b, math.inf)]
    zs += [2.0 ** k for k in range(-10, 1021, 3)] + [2.0 ** 1021, 2.0 ** 1022, 2.0 ** 1023, math.inf]
    return sorted(set(zs))


def _one(z):
    mp.mp.dps = 60 if z < 0 else 50
    q, _, dl = lr.tail(mp.mpf(z))
    return mp.nstr(q, 25), mp.nstr(dl, 25)


def main():
    zs = abscissae()
    with mpc.Pool(min(8, os.cpu_count() or 1)) as pool:
        out = pool.map(_one, zs, chunksize=8)
    mp.mp.dps = 50
    t1 = [[L, th, 0.05, mp.nstr(lr.table1_check(L, th), 6)] for L, th in ((10, 0.040), (100, 0.036), (1000, 0.034), (10000, 0.031))]
    for row in t1:
        print("Table 1: L = %d, threshold %.3f -> %s" % (row[0], row[1], row[3]))
    doc = dict(about="Q(z) = (1/pi) int_0^inf exp(-t z - (2/pi) t log t) sin(2 t)/t dt and d log Q/dz, mpmath, 25 digits; tools/make_landau_golden.py",
               z=[float.hex(z) if z != math.inf else "inf" for z in zs], Q=[o[0] for o in out], dlogQ_dz=[o[1] for o in out],
               table1=[dict(L=r[0], threshold=r[1], expected=r[2], tail=r[3]) for r in t1])
    path = os.path.join(ROOT, "tests", "golden", "landau_tail.json")
    with open(path, "w") as f:
        json.dump(doc, f, indent=0)
    print("wrote", path, len(zs), "abscissae")


if __name__ == "__main__":
    main()
