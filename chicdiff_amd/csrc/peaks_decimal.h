// peaks_decimal.h — a decimal token -> the correctly rounded double (round to nearest, ties to even), decided with integers alone.
// The rule for the token stands above chicdiff_hip_peaks_parse_dev in include/chicdiff_hip.h.
//
// A token is read as (sign, w, q): w = its digits up to the last non-zero one as an integer with the leading zeros dropped, q the
// decimal exponent that remains, value = w * 10^q.  With at most 19 such digits w < 10^19 < 2^64, and for |q| <= kPow5Max = 39:
//   q >= 0   w * 5^q < 2^64 * 2^91: a 192-bit integer, computed exactly; the value is that integer times 2^q, so its 53 leading
//            bits, the bit behind them and "anything non-zero further down" decide the rounding.
//   q <  0   value = w / 5^k * 2^-k, k = -q.  With s chosen from the bit lengths so that Q = floor(w * 2^s / 5^k) has 54 or 55
//            bits, Q and "remainder non-zero" decide the rounding.  Q comes from one fp64 quotient (off by a few units at most),
//            then the remainder w * 2^s - Q * 5^k is formed exactly and Q stepped until 0 <= remainder < 5^k: no wide division.
// Every result is a normal double (10^-39 <= value < 2^64 * 10^39), so no subnormal or overflow case arises here.  A token outside
// this domain — more digits, a larger exponent — is not decided here: the scan reports it as SLOW and the host settles it.
// In particular a token with at most 17 significant digits and |q| <= 22 is always decided here.
#pragma once
#include <math.h>
#include <stdint.h>

#include "pow5_table.h"

#if defined(__HIPCC__)
#define PK_HD __host__ __device__
#else
#define PK_HD
#endif

namespace cd {

constexpr int kPkMaxDigits = 19;

PK_HD inline int pk_bitlen64(uint64_t x) {  // x != 0
#if defined(__HIP_DEVICE_COMPILE__)
    return 64 - __clzll((long long)x);
#else
    return 64 - __builtin_clzll(x);
#endif
}

PK_HD inline void pk_mul64(uint64_t a, uint64_t b, uint64_t &lo, uint64_t &hi) {
#if defined(__HIP_DEVICE_COMPILE__)
    lo = a * b;
    hi = __umul64hi(a, b);
#else
    const unsigned __int128 p = (unsigned __int128)a * b;
    lo = (uint64_t)p;
    hi = (uint64_t)(p >> 64);
#endif
}

PK_HD inline double pk_bits_to_double(uint64_t b) {
#if defined(__HIP_DEVICE_COMPILE__)
    return __longlong_as_double((long long)b);
#else
    double d;
    __builtin_memcpy(&d, &b, 8);
    return d;
#endif
}

// (Q + f) * 2^e with 2^53 <= Q < 2^55, 0 <= f < 1 and sticky = (f != 0) -> the nearest double, ties to even
PK_HD inline double pk_round_pack(uint64_t Q, bool sticky, int e, bool neg) {
    bool round;
    if (Q >> 54) {
        sticky = sticky || (Q & 1);
        round = (Q >> 1) & 1;
        Q >>= 2;
        e += 2;
    } else {
        round = Q & 1;
        Q >>= 1;
        e += 1;
    }
    if (round && (sticky || (Q & 1))) Q++;
    if (Q >> 53) {
        Q >>= 1;
        e++;
    }
    const uint64_t bits = ((uint64_t)neg << 63) | ((uint64_t)(e + 52 + 1023) << 52) | (Q & ((1ull << 52) - 1));
    return pk_bits_to_double(bits);
}

// w * 10^q, w != 0, |q| <= kPow5Max; pow5 = the table (kPow5 itself, or a copy in LDS).  *ok = false: not decided (never seen: the
// step loop below is bounded although the estimate's error bound makes a few steps enough).
PK_HD inline double pk_decimal_value(uint64_t w, int q, bool neg, const uint64_t (*pow5)[2], bool *ok) {
    *ok = true;
    if (q >= 0) {
        const uint64_t d0 = pow5[q][0], d1 = pow5[q][1];
        uint64_t p0, h0, l1, p2;
        pk_mul64(w, d0, p0, h0);
        pk_mul64(w, d1, l1, p2);
        uint64_t p1 = h0 + l1;
        p2 += p1 < h0;
        const int L = p2 ? 128 + pk_bitlen64(p2) : (p1 ? 64 + pk_bitlen64(p1) : pk_bitlen64(p0));
        if (L <= 55) return pk_round_pack(p0 << (55 - L), false, q + L - 55, neg);
        const int r = L - 55, wr = r >> 6, br = r & 63;
        bool sticky = false;
        uint64_t a0 = p0, a1 = p1;
        if (wr == 1) {
            sticky = p0 != 0;
            a0 = p1; a1 = p2;
        } else if (wr == 2) {
            sticky = (p0 | p1) != 0;
            a0 = p2; a1 = 0;
        }
        uint64_t Q = a0;
        if (br) {
            sticky = sticky || (a0 & ((1ull << br) - 1));
            Q = (a0 >> br) | (a1 << (64 - br));
        }
        return pk_round_pack(Q, sticky, q + r, neg);
    }
    const int k = -q;
    uint64_t d0 = pow5[k][0], d1 = pow5[k][1];
    const int lw = pk_bitlen64(w), lD = d1 ? 64 + pk_bitlen64(d1) : pk_bitlen64(d0);
    const int s = 54 - (lw - lD);  // w * 2^s / 5^k lies in (2^53, 2^55)
    uint64_t n0, n1 = 0, n2 = 0;
    if (s >= 0) {  // N = w << s: at most 54 + lD <= 145 bits
        const int ws = s >> 6, bs = s & 63;
        const uint64_t lo = w << bs, hi = bs ? w >> (64 - bs) : 0;
        if (ws == 0) { n0 = lo; n1 = hi; }
        else if (ws == 1) { n0 = 0; n1 = lo; n2 = hi; }
        else { n0 = 0; n1 = 0; n2 = lo; }
    } else {  // D = 5^k << -s: lD - s = lw - 54 <= 10 bits
        n0 = w;
        d0 <<= -s;
    }
    const double xn = ldexp((double)w, s > 0 ? s : 0);
    const double xd = (double)d1 * 18446744073709551616.0 + (double)d0;
    uint64_t Q = (uint64_t)(xn / xd);
    // R = N - Q * D, modulo 2^192; the estimate is within a few units of the quotient, so |R| is a few D
    uint64_t m0, mh0, ml1, m2;
    pk_mul64(Q, d0, m0, mh0);
    pk_mul64(Q, d1, ml1, m2);
    uint64_t m1 = mh0 + ml1;
    m2 += m1 < mh0;
    uint64_t r0 = n0 - m0;
    uint64_t b = n0 < m0;
    uint64_t r1 = n1 - m1 - b;
    b = (n1 < m1) || (n1 == m1 && b);
    uint64_t r2 = n2 - m2 - b;
    int steps = 0;
    while ((r2 >> 63) && steps < 64) {  // R < 0: Q too large
        const uint64_t t0 = r0 + d0;
        uint64_t c = t0 < r0;
        const uint64_t t1 = r1 + d1 + c;
        c = (t1 < r1) || (t1 == r1 && c);
        r0 = t0; r1 = t1; r2 += c;
        Q--;
        steps++;
    }
    while (!(r2 >> 63) && (r2 || r1 > d1 || (r1 == d1 && r0 >= d0)) && steps < 64) {  // R >= D: Q too small
        const uint64_t t0 = r0 - d0;
        uint64_t c = r0 < d0;
        const uint64_t t1 = r1 - d1 - c;
        c = (r1 < d1) || (r1 == d1 && c);
        r0 = t0; r1 = t1; r2 -= c;
        Q++;
        steps++;
    }
    if (steps >= 64 || !(Q >> 53) || (Q >> 55)) {
        *ok = false;
        return 0.0;
    }
    return pk_round_pack(Q, (r0 | r1 | r2) != 0, -k - s, neg);
}

enum { PK_OK = 0, PK_MALFORMED = 1, PK_SLOW = 2 };

PK_HD inline bool pk_digit(unsigned char c) { return c >= '0' && c <= '9'; }

// One decimal field from p on, read through rd (rd.at(p), rd.line_end(c, p)); p ends on the field's terminator: the separator or the
// line's end.  Empty or exactly NA -> NaN.  PK_SLOW: a well-formed token this header does not decide (*out = NaN meanwhile).
template <class Reader>
PK_HD inline int pk_scan_decimal(const Reader &rd, int64_t &p, unsigned char sep, const uint64_t (*pow5)[2], double *out) {
    unsigned char c = rd.at(p);
    auto term = [&](unsigned char ch, int64_t at) { return ch == sep || rd.line_end(ch, at); };
    *out = pk_bits_to_double(0x7ff8000000000000ull);
    if (term(c, p)) return PK_OK;
    if (c == 'N') {
        if (rd.at(p + 1) != 'A') return PK_MALFORMED;
        p += 2;
        return term(rd.at(p), p) ? PK_OK : PK_MALFORMED;
    }
    bool neg = false;
    if (c == '+' || c == '-') {
        neg = c == '-';
        c = rd.at(++p);
    }
    uint64_t w = 0;
    int nd = 0, pend = 0, nfrac = 0;
    bool any = false, slow = false;
    auto fold = [&](int d) {
        if (d == 0) {
            if (w != 0) {
                if (pend < (1 << 20)) pend++;
                else slow = true;
            }
            return;
        }
        if (slow || nd + pend + 1 > kPkMaxDigits) {
            slow = true;
            return;
        }
        nd += pend + 1;
        for (; pend > 0; pend--) w *= 10;
        w = w * 10 + (uint64_t)d;
    };
    while (pk_digit(c)) {
        any = true;
        fold(c - '0');
        c = rd.at(++p);
    }
    if (c == '.') {
        c = rd.at(++p);
        while (pk_digit(c)) {
            any = true;
            if (nfrac < (1 << 20)) nfrac++;
            else slow = true;
            fold(c - '0');
            c = rd.at(++p);
        }
    }
    if (!any) return PK_MALFORMED;
    int ex = 0;
    if (c == 'e' || c == 'E') {
        c = rd.at(++p);
        bool eneg = false;
        if (c == '+' || c == '-') {
            eneg = c == '-';
            c = rd.at(++p);
        }
        if (!pk_digit(c)) return PK_MALFORMED;
        while (pk_digit(c)) {
            if (ex < 100000) ex = ex * 10 + (c - '0');
            c = rd.at(++p);
        }
        if (eneg) ex = -ex;
    }
    if (!term(c, p)) return PK_MALFORMED;
    if (w == 0) {
        *out = pk_bits_to_double((uint64_t)neg << 63);
        return PK_OK;
    }
    const int q = ex + pend - nfrac;
    if (slow || q > kPow5Max || q < -kPow5Max) return PK_SLOW;
    bool ok;
    const double v = pk_decimal_value(w, q, neg, pow5, &ok);
    if (!ok) return PK_SLOW;
    *out = v;
    return PK_OK;
}

}  // namespace cd
