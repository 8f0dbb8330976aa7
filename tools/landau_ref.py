"""The upper tail Q(z) of the Landau distribution behind harmonicmeanp::p.hmp (Wilson 2019, PNAS 116:1195, eq. 4), in mpmath:
what tools/make_landau_table.py fits and tools/make_landau_golden.py tabulates.

    Q(z) = (1 / pi) int_0^inf exp(-t z - (2 / pi) t log t) sin(2 t) / t dt                                (the Laplace form)

is the tail of the stable law S(alpha = 1, beta = 1) with characteristic function exp(-|t| - i (2 / pi) t log|t|).  The Laplace
form is well conditioned for z >= 0 and cancels for z < 0 (its integrand grows like exp(|z| t)).  There Zolotarev's integral of
the same law is used, whose integrand is positive and which gives 1 - Q, not Q:

    1 - Q(z) = (1 / pi) int_0^pi exp(-eps V(phi)) dphi,   eps = exp(-pi z / 2),   V(phi) = (2 / pi) (phi / sin phi) exp(-phi cot phi)

The two forms are independent of each other; agree() compares them where both work.  -dQ/dz has the same two forms (one factor
t, or eps V pi / 2, more).  All functions take and return mpf at the precision the caller has set."""
import mpmath as mp


def _breaks(hi):
    pts, x = [mp.mpf(0)], mp.mpf(1)
    while x < hi:
        pts.append(x)
        x *= 4
    return pts + [mp.inf]


def tail_laplace(z):
    """(Q, -dQ/dz) from the Laplace form, z >= 0.  t = u / max(z, 1): the integrand decays like exp(-u) at least."""
    z = mp.mpf(z)
    sc = max(z, mp.mpf(1))
    a, c = z / sc, 2 / mp.pi

    def e(u):
        t = u / sc
        return mp.exp(-a * u - c * t * mp.log(t)) if t else mp.mpf(1)

    # both integrands are scaled to order one: quad stops on an ABSOLUTE error estimate, which says nothing about an integrand of 1e-90
    def fq(u):
        t = u / sc
        return e(u) * mp.sin(2 * t) / t if u else mp.mpf(2)

    def fd(u):
        t = u / sc
        return e(u) * mp.sin(2 * t) / t * u if u else mp.mpf(0)

    br = _breaks(256)
    return mp.quad(fq, br) / (mp.pi * sc), mp.quad(fd, br) / (mp.pi * sc * sc)


def _V(phi, cap=None):
    """V(phi); None where V > cap (towards phi = pi it grows like exp(pi / (pi - phi)): not to be exponentiated twice)."""
    lv = mp.log((2 / mp.pi) * (phi / mp.sin(phi))) - phi * mp.cot(phi)
    if cap is not None and lv > mp.log(cap):
        return None
    return mp.exp(lv)


def head_zolotarev(z):
    """(1 - Q, -dQ/dz) from Zolotarev's form; any z, meant for z < 0.  Below z = -6 the head is under exp(-2000): (0, 0)."""
    z = mp.mpf(z)
    if z < -6:
        return mp.mpf(0), mp.mpf(0)
    eps = mp.exp(-mp.pi * z / 2)
    v0 = 2 / (mp.pi * mp.e)

    cap = 10000 / eps   # exp(-10000) is nothing at any precision used here

    def fh(phi):
        v = _V(phi, cap) if phi else v0
        return mp.exp(-eps * v) if v is not None else mp.mpf(0)

    def fd(phi):
        v = _V(phi, cap) if phi else v0
        return v * mp.exp(-eps * v) if v is not None else mp.mpf(0)

    # the integrand falls from exp(-eps V(0)) at phi = 0 to nothing at phi = pi, faster the larger eps is
    br = [mp.mpf(0)] + [mp.pi * mp.mpf(k) / 16 for k in (1, 2, 4, 6, 8, 10, 12, 14, 15)] + [mp.pi]
    return mp.quad(fh, br) / mp.pi, eps / 2 * mp.quad(fd, br)


def tail(z):
    """(Q, 1 - Q, d log Q / dz): Zolotarev's form below zero (1 - Q is formed directly), the Laplace form from zero on."""
    z = mp.mpf(z)
    if z == mp.inf:
        return mp.mpf(0), mp.mpf(1), mp.mpf(0)
    if z < 0:
        h, d = head_zolotarev(z)
        return 1 - h, h, -d / (1 - h)
    q, d = tail_laplace(z)
    return q, 1 - q, -d / q


def agree(zs=(-2, -1, -0.5, 0, 0.5, 1, 3)):
    """Largest relative difference of the two forms' Q and dQ/dz over zs (the Laplace form is pushed below zero for this)."""
    worst = mp.mpf(0)
    for z in zs:
        q, d = tail_laplace(z) if z >= 0 else _laplace_negative(z)
        h, dz = head_zolotarev(z)
        worst = max(worst, abs(q - (1 - h)) / q, abs(d - dz) / d)
    return worst


def _laplace_negative(z):
    z, c = mp.mpf(z), 2 / mp.pi
    e = lambda t: mp.exp(-z * t - c * t * mp.log(t)) if t else mp.mpf(1)
    br = _breaks(64)
    return (mp.quad(lambda t: e(t) * mp.sin(2 * t) / t if t else mp.mpf(2), br) / mp.pi,
            mp.quad(lambda t: e(t) * mp.sin(2 * t), br) / mp.pi)


def series_coefficients(nterms):
    """Q(z) = (1 / z) sum_{n < nterms} z^-n P_n(log z) + ..., the expansion of the Laplace form for z -> inf: rows[n][j] is the
    coefficient of (log z)^j in P_n.  From exp(-(2 / pi) t log t) sin(2 t) / t = sum_k (-(2 / pi) t log t)^k / k! *
    sum_m (-1)^m 2^(2 m + 1) t^(2 m) / (2 m + 1)!  and  int_0^inf exp(-t z) t^n (log t)^k dt = d^k/ds^k [Gamma(s + 1) z^(-s - 1)] at s = n."""
    rows = []
    for n in range(nterms):
        row = [mp.mpf(0)] * (n + 1)
        dg = [mp.diff(mp.gamma, n + 1, j) if j else mp.gamma(n + 1) for j in range(n + 1)]
        for m in range(n // 2 + 1):
            k = n - 2 * m
            w = (-2 / mp.pi) ** k / mp.factorial(k) * (-1) ** m * mp.mpf(2) ** (2 * m + 1) / mp.factorial(2 * m + 1) / mp.pi
            for j in range(k + 1):   # C(k, j) Gamma^(j)(n + 1) (-log z)^(k - j)
                row[k - j] += w * mp.binomial(k, j) * dg[j] * (-1) ** (k - j)
        rows.append(row)
    return rows


def series(rows, z):
    z = mp.mpf(z)
    L, w = mp.log(z), 1 / z
    return w * sum(w ** n * mp.polyval(list(reversed(r)), L) for n, r in enumerate(rows))


def table1_check(L, threshold):
    """Tail probability of the paper's Table 1 threshold: the harmonic mean p equals `threshold` when x = 1 / threshold."""
    c = 1 + mp.digamma(1) - mp.log(2 / mp.pi)
    return tail((1 / mp.mpf(threshold) - (mp.log(L) + c)) / (mp.pi / 2))[0]
