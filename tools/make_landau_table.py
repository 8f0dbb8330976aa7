#!/usr/bin/env python3
"""Generate chicdiff_amd/csrc/landau_table.h: the coefficients behind devmath.h landau_tail(z), the Landau tail Q(z) that
harmonicmeanp::p.hmp evaluates (tools/landau_ref.py has the formula and its two quadratures).  Run by hand from the repository
root (some minutes on 8 cores); the build never runs it.

    z <= ONE                 Q = 1: 1 - Q < 2^-54 there (printed below)
    ONE <= z < 2             NUNI intervals of width 1/4
    2 <= z < CUT = 2^(NOCT+1)   four intervals per octave, chosen by the exponent and the two top mantissa bits of z: they
                             grow geometrically, as the function flattens
    z >= CUT                 Q = (1 / z) sum_{n < NTERMS} z^-n P_n(log z), the leading terms of the expansion for z -> inf

On an interval [a, b] the fit is a polynomial of degree DEG in s = (z - (a + b) / 2) / ((b - a) / 2): the interpolant of Q in
the Chebyshev nodes, converted to powers of s and rounded to fp64.  The transform of Q is the identity: Q changes by less than a
factor 1.4 over an interval, so an error relative to the polynomial's size is an error relative to Q.  END holds Q at the
interval bounds, correctly rounded: the evaluation clamps to [END[i + 1], END[i]], which makes it non-increasing across every
seam whatever the last bits of two neighbouring polynomials do.

The approximation error (rounded coefficients, exact arithmetic) is measured between the nodes and printed in units of 2^-53 Q;
the run fails if it reaches 1/4 of a unit, i.e. if it is not well below the rounding of the fp64 evaluation.  The constant
coefficient is stored as two doubles (hi, lo) for that."""
import json
import multiprocessing as mpc
import os
import sys

import mpmath as mp

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import landau_ref as lr  # noqa: E402

DPS = 40
ONE = -3.5
NUNI = 22
NOCT = int(os.environ.get("LANDAU_NOCT", "6"))
DEG = int(os.environ.get("LANDAU_DEG", "15"))
NTERMS = int(os.environ.get("LANDAU_NTERMS", "10"))
CUT = 2.0 ** (NOCT + 1)
OUT = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "chicdiff_amd", "csrc", "landau_table.h")


def bounds():
    b = [ONE + 0.25 * i for i in range(NUNI + 1)]
    for e in range(1, NOCT + 1):
        b += [2.0 ** e * (1 + q / 4) for q in range(1, 5)]
    return b


def _q(z):
    mp.mp.dps = DPS
    return lr.tail(mp.mpf(z))[0]


def _head(z):
    mp.mp.dps = DPS
    return lr.tail(mp.mpf(z))[1]


def cheb_to_powers(c):
    """Chebyshev coefficients -> coefficients of powers of s (low to high)."""
    n = len(c)
    T = [[mp.mpf(1)], [mp.mpf(0), mp.mpf(1)]]
    for k in range(2, n):
        t = [mp.mpf(0)] + [2 * x for x in T[k - 1]]
        for j, x in enumerate(T[k - 2]):
            t[j] -= x
        T.append(t)
    out = [mp.mpf(0)] * n
    for k in range(n):
        for j, x in enumerate(T[k]):
            out[j] += c[k] * x
    return out


def main():
    mp.mp.dps = DPS
    b = bounds()
    nint = len(b) - 1
    assert nint == NUNI + 4 * NOCT and b[NUNI] == 2.0 and b[-1] == CUT
    N = DEG + 1
    nodes = [mp.cos(mp.pi * (2 * j + 1) / (2 * N)) for j in range(N)]
    checks = [mp.cos(mp.pi * j / N) for j in range(1, N)]   # between the nodes
    zs = []
    for i in range(nint):
        c, h = (mp.mpf(b[i]) + mp.mpf(b[i + 1])) / 2, (mp.mpf(b[i + 1]) - mp.mpf(b[i])) / 2
        zs += [c + h * s for s in nodes + checks]
    beyond = [CUT, CUT * 1.5, CUT * 2, CUT * 4, CUT * 16, CUT * 256]
    cache = os.environ.get("LANDAU_CACHE")   # optional: keep the quadratures between runs that only change the output
    if cache and os.path.exists(cache):
        vals = [mp.mpf(v) for v in json.load(open(cache))]
        assert len(vals) == len(zs + b + beyond) + 1
    else:
        with mpc.Pool(min(8, os.cpu_count() or 1)) as pool:
            vals = pool.map(_q, zs + b + beyond, chunksize=4) + pool.map(_head, [ONE])
        if cache:
            json.dump([mp.nstr(v, DPS) for v in vals], open(cache, "w"))
    head_one = vals.pop()
    per = N + len(checks)
    ends = vals[nint * per:nint * per + len(b)]
    far = vals[nint * per + len(b):]
    print(f"z <= {ONE}: 1 - Q = {mp.nstr(head_one, 5)} = 2^{mp.nstr(mp.log(head_one, 2), 5)}")
    assert head_one < mp.mpf(2) ** -54
    coef, worst = [], mp.mpf(0)
    for i in range(nint):
        f = vals[i * per:i * per + N]
        ch = [(2 if k else 1) * sum(f[j] * mp.cos(mp.pi * k * (2 * j + 1) / (2 * N)) for j in range(N)) / N for k in range(N)]
        exact = cheb_to_powers(ch)
        c0 = float(exact[0])   # s^0 is kept as hi + lo: rounding it to one double alone would cost up to 1/2 unit
        row = [c0, float(exact[0] - mp.mpf(c0))] + [float(x) for x in exact[1:]]
        pw = [mp.mpf(row[0]) + mp.mpf(row[1])] + [mp.mpf(x) for x in row[2:]]
        err = max(abs(mp.polyval(list(reversed(pw)), s) - q) / q for s, q in zip(checks, vals[i * per + N:(i + 1) * per]))
        units = err * mp.mpf(2) ** 53
        worst = max(worst, units)
        print(f"interval {i:2d} [{b[i]:g}, {b[i + 1]:g}): approximation error {mp.nstr(units, 3)} units of 2^-53 Q")
        coef.append(row)
    print(f"worst approximation error {mp.nstr(worst, 3)} units of 2^-53 Q at degree {DEG}")
    assert worst < 0.25, "raise DEG"
    rows = lr.series_coefficients(NTERMS)
    p0 = float(rows[0][0])   # 2 / pi, kept as hi + lo like the polynomials' constant coefficients
    flat = [p0, float(rows[0][0] - mp.mpf(p0))] + [float(x) for r in rows[1:] for x in r]
    rows_d = [[mp.mpf(flat[0]) + mp.mpf(flat[1])]] + [[mp.mpf(float(x)) for x in r] for r in rows[1:]]
    trunc = mp.mpf(0)
    for z, q in zip(beyond, far):
        e = abs(lr.series(rows_d, z) - q) / q * mp.mpf(2) ** 53
        trunc = max(trunc, e)
        print(f"expansion, {NTERMS} terms, z = {z:g}: truncation error {mp.nstr(e, 3)} units of 2^-53 Q")
    print(f"cut-over at z = {CUT:g}: truncation error at most {mp.nstr(trunc, 3)} units of 2^-53 Q (largest at the cut-over)")
    assert trunc < 0.25, "raise NOCT or NTERMS"
    hx = lambda x: float.hex(float(x))
    with open(OUT, "w") as f:
        f.write("// landau_table.h — GENERATED by tools/make_landau_table.py; do not edit.\n")
        f.write("// Q(z), the upper tail of the Landau distribution of harmonicmeanp::p.hmp: see devmath.h landau_tail().\n")
        f.write(f"// Approximation error {mp.nstr(worst, 3)}, truncation error of the expansion {mp.nstr(trunc, 3)} units of 2^-53 Q at most.\n")
        f.write("#pragma once\n\n")
        f.write(f"#define CD_LANDAU_ONE {hx(ONE)}\n#define CD_LANDAU_NUNI {NUNI}\n#define CD_LANDAU_NOCT {NOCT}\n")
        f.write(f"#define CD_LANDAU_NINT {nint}\n#define CD_LANDAU_DEG {DEG}\n#define CD_LANDAU_CUT {hx(CUT)}\n#define CD_LANDAU_NTERMS {NTERMS}\n")
        f.write("// per interval: s^0 as (hi, lo), then the coefficients of s^1 .. s^DEG\n#define CD_LANDAU_COEF_INIT \\\n")
        f.write(", \\\n".join("    {" + ", ".join(hx(x) for x in row) + "}" for row in coef) + "\n")
        f.write("// Q at the NINT + 1 interval bounds\n#define CD_LANDAU_END_INIT \\\n")
        f.write(", \\\n".join("    " + hx(x) for x in ends) + "\n")
        f.write("// expansion: P_0 = 2 / pi as (hi, lo), then P_1's two coefficients, ... (powers of log z, low to high)\n#define CD_LANDAU_SERIES_INIT \\\n")
        f.write("    " + ", ".join(hx(x) for x in flat) + "\n")
    print("wrote", OUT)


if __name__ == "__main__":
    main()
