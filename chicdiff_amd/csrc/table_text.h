// table_text.h — one cell of a table as text, decided with integers alone: a double -> Python's repr(float) (what pandas' to_csv writes for a
// float64 column without float_format), an integer -> its decimal digits.  The rule stands above chicdiff_hip_table_text_dev in
// include/chicdiff_hip.h.  Host and device code: table_text_kernels.hip runs it per lane, table_api.hip and tests/table_text_host.cpp
// on the host.  No floating-point arithmetic, no printf, no library call.
//
// double -> (digits, exponent): the Schubfach conversion (R. Giulietti, "The Schubfach way to render doubles", 2020).  v = c * 2^q; with
// k = floor(log10(2^q)) (of 3/4 * 2^q where the interval below v is half as wide: c = 2^52, q > -1074) the three numbers 4c - 2 (or - 1),
// 4c, 4c + 2 are scaled by 10^-k through ONE 64 x 128-bit product each against g(-k) of pow10_table.h, the bits that fall off kept as a
// sticky bit ("round to odd").  That is exact enough to decide which of the two k-digit neighbours of v, or of the two one digit
// shorter, lie inside the rounding interval of v and which is closer, ties to the even digit.  The result read back is v, no shorter
// digit string reads back as v, and among the shortest it is the closest; trailing zeros are then dropped.
//
// (digits, exponent) -> text, float_repr_style "short": decpt = exponent + number of digits; -4 < decpt <= 16 positional, always with
// a fractional part (5.0, -0.0, 0.0001, 9999999999999998.0); otherwise d[.ddd]e+XX / e-XX with at least two exponent digits.  NaN of
// any sign and payload: no byte.  inf, -inf.  A cell is at most kTtMaxCell = 24 bytes (-2.2250738585072014e-308).
//
// The text is written through a sink, sink.put(position, byte): the length of the cell and the place of every byte are known before
// the first digit is formed, so the digits are taken off the low end of the integer (constant divisions) and need no buffer.
#pragma once
#include <stdint.h>

#include "pow10_table.h"

#if defined(__HIPCC__)
#define TT_HD __host__ __device__
#else
#define TT_HD
#endif

namespace cd {

constexpr int kTtMaxCell = 24;

TT_HD inline void tt_mul64(uint64_t a, uint64_t b, uint64_t &lo, uint64_t &hi) {
#if defined(__HIP_DEVICE_COMPILE__)
    lo = a * b;
    hi = __umul64hi(a, b);
#else
    const unsigned __int128 p = (unsigned __int128)a * b;
    lo = (uint64_t)p;
    hi = (uint64_t)(p >> 64);
#endif
}

// floor(cp * g / 2^128), bit 0 set when anything non-zero fell off below it (g = {low, high}, cp < 2^64)
TT_HD inline uint64_t tt_round_to_odd(const uint64_t g[2], uint64_t cp) {
    uint64_t xl, xh, yl, yh;
    tt_mul64(cp, g[0], xl, xh);
    tt_mul64(cp, g[1], yl, yh);
    const uint64_t y0 = yl + xh;
    const uint64_t y1 = yh + (y0 < yl);
    return y1 | (uint64_t)(y0 > 1);
}

TT_HD inline int tt_ndigits(uint64_t v) {  // decimal digits of v, v != 0 -> 1 .. 20
    int n = 1;
    if (v >= 10000000000000000ull) { v /= 10000000000000000ull; n += 16; }
    if (v >= 100000000ull) { v /= 100000000ull; n += 8; }
    if (v >= 10000ull) { v /= 10000ull; n += 4; }
    if (v >= 100ull) { v /= 100ull; n += 2; }
    if (v >= 10ull) n += 1;
    return n;
}

struct TtDecimal {
    uint64_t digits;  // != 0, last digit != 0
    int exp10;        // value = digits * 10^exp10
    int nd;           // decimal digits of `digits`, 1 .. 17
};

TT_HD inline TtDecimal tt_strip(uint64_t d, int e) {
    while (true) {
        const uint64_t q = d / 10;
        if (q * 10 != d) break;
        d = q;
        e++;
    }
    return TtDecimal{d, e, tt_ndigits(d)};
}

// frac = the 52 fraction bits, bexp = the 11 exponent bits (not 2047, and not both zero); pow10 = kPow10 (or a copy of it)
TT_HD inline TtDecimal tt_shortest(uint64_t frac, int bexp, const uint64_t (*pow10)[2]) {
    uint64_t c;
    int q;
    if (bexp != 0) {
        c = (1ull << 52) | frac;
        q = bexp - 1075;
        if (q <= 0 && q > -53 && (c & ((1ull << -q) - 1)) == 0) return tt_strip(c >> -q, 0);  // an integer below 2^53
    } else {
        c = frac;
        q = -1074;
    }
    const bool even = (c & 1) == 0;
    const bool narrow = frac == 0 && bexp > 1;  // the interval below v is half as wide as the one above
    const uint64_t cbl = 4 * c - 2 + (narrow ? 1 : 0), cb = 4 * c, cbr = 4 * c + 2;
    const int k = (q * 1262611 - (narrow ? 524031 : 0)) >> 22;  // floor(log10(2^q)), floor(log10(3/4 * 2^q))
    const int h = q + ((-k * 1741647) >> 19) + 1;               // q + floor(log2(10^-k)) + 1: 1 .. 4
    const uint64_t *g = pow10[-k - kPow10Min];
    const uint64_t vbl = tt_round_to_odd(g, cbl << h), vb = tt_round_to_odd(g, cb << h), vbr = tt_round_to_odd(g, cbr << h);
    const uint64_t lower = vbl + (even ? 0 : 1), upper = vbr - (even ? 0 : 1);
    const uint64_t s = vb >> 2;
    if (s >= 10) {  // one digit fewer?
        const uint64_t sp = s / 10;
        const bool up_in = lower <= 40 * sp, wp_in = 40 * sp + 40 <= upper;
        if (up_in != wp_in) return tt_strip(sp + (wp_in ? 1 : 0), k + 1);
    }
    const bool u_in = lower <= 4 * s, w_in = 4 * s + 4 <= upper;
    if (u_in != w_in) return tt_strip(s + (w_in ? 1 : 0), k);
    const uint64_t mid = 4 * s + 2;
    const bool up = vb > mid || (vb == mid && (s & 1) != 0);
    return tt_strip(s + (up ? 1 : 0), k);
}

// ---- the layout of a double's cell ------------------------------------------------------------------------------------------
struct TtDoubleLayout {
    int len;       // bytes of the cell
    int kind;      // 0 nothing (NaN), 1 inf, 2 zero, 3 positional, 4 exponent form
    bool neg;
    TtDecimal d;   // kinds 3 and 4
    int decpt;     // kinds 3 and 4: value = 0.d1 d2 ... * 10^decpt
};

TT_HD inline TtDoubleLayout tt_double_layout(uint64_t bits, const uint64_t (*pow10)[2]) {
    TtDoubleLayout L{0, 0, (bits >> 63) != 0, TtDecimal{0, 0, 0}, 0};
    const uint64_t frac = bits & ((1ull << 52) - 1);
    const int bexp = (int)((bits >> 52) & 2047);
    const int sign = L.neg ? 1 : 0;
    if (bexp == 2047) {
        if (frac != 0) return L;
        L.kind = 1;
        L.len = sign + 3;
        return L;
    }
    if (bexp == 0 && frac == 0) {
        L.kind = 2;
        L.len = sign + 3;
        return L;
    }
    L.d = tt_shortest(frac, bexp, pow10);
    const int nd = L.d.nd, decpt = L.d.exp10 + nd;
    L.decpt = decpt;
    if (decpt > -4 && decpt <= 16) {
        L.kind = 3;
        L.len = sign + (decpt <= 0 ? 2 - decpt + nd : (decpt < nd ? nd + 1 : decpt + 2));
    } else {
        const int e = decpt - 1, ae = e < 0 ? -e : e;
        L.kind = 4;
        L.len = sign + nd + (nd > 1 ? 1 : 0) + 2 + (ae >= 100 ? 3 : 2);
    }
    return L;
}

TT_HD inline int tt_double_len(uint64_t bits, const uint64_t (*pow10)[2]) { return tt_double_layout(bits, pow10).len; }

// the cell of `bits` from position p on; returns its length
template <class Sink>
TT_HD inline int tt_put_double(uint64_t bits, const uint64_t (*pow10)[2], Sink &sink, int p) {
    const TtDoubleLayout L = tt_double_layout(bits, pow10);
    if (L.kind == 0) return 0;
    int b = p;
    if (L.neg) sink.put(b++, '-');
    if (L.kind == 1) {
        sink.put(b, 'i'); sink.put(b + 1, 'n'); sink.put(b + 2, 'f');
        return L.len;
    }
    if (L.kind == 2) {
        sink.put(b, '0'); sink.put(b + 1, '.'); sink.put(b + 2, '0');
        return L.len;
    }
    const int nd = L.d.nd, decpt = L.decpt;
    uint64_t v = L.d.digits;
    if (L.kind == 3) {
        if (decpt <= 0) {  // 0.000ddd
            sink.put(b, '0'); sink.put(b + 1, '.');
            for (int z = 0; z < -decpt; z++) sink.put(b + 2 + z, '0');
            b += 2 - decpt;
            for (int i = nd - 1; i >= 0; i--) {
                const uint64_t t = v / 10;
                sink.put(b + i, (unsigned char)('0' + (int)(v - 10 * t)));
                v = t;
            }
        } else if (decpt < nd) {  // dd.ddd
            for (int i = nd - 1; i >= 0; i--) {
                const uint64_t t = v / 10;
                sink.put(b + i + (i >= decpt ? 1 : 0), (unsigned char)('0' + (int)(v - 10 * t)));
                v = t;
            }
            sink.put(b + decpt, '.');
        } else {  // ddd000.0
            for (int i = nd - 1; i >= 0; i--) {
                const uint64_t t = v / 10;
                sink.put(b + i, (unsigned char)('0' + (int)(v - 10 * t)));
                v = t;
            }
            for (int z = nd; z < decpt; z++) sink.put(b + z, '0');
            sink.put(b + decpt, '.'); sink.put(b + decpt + 1, '0');
        }
        return L.len;
    }
    // d[.ddd]e+XX
    for (int i = nd - 1; i >= 0; i--) {
        const uint64_t t = v / 10;
        sink.put(b + (i == 0 ? 0 : i + 1), (unsigned char)('0' + (int)(v - 10 * t)));
        v = t;
    }
    if (nd > 1) sink.put(b + 1, '.');
    b += nd + (nd > 1 ? 1 : 0);
    int e = decpt - 1;
    sink.put(b, 'e');
    sink.put(b + 1, e < 0 ? '-' : '+');
    if (e < 0) e = -e;
    b += 2;
    if (e >= 100) {
        sink.put(b++, (unsigned char)('0' + e / 100));
        e %= 100;
    }
    sink.put(b, (unsigned char)('0' + e / 10));
    sink.put(b + 1, (unsigned char)('0' + e % 10));
    return L.len;
}

// ---- integers ---------------------------------------------------------------------------------------------------------------------
TT_HD inline int tt_int_len(int64_t x) {
    const uint64_t mag = x < 0 ? 0 - (uint64_t)x : (uint64_t)x;
    return (x < 0 ? 1 : 0) + (mag ? tt_ndigits(mag) : 1);
}

template <class Sink>
TT_HD inline int tt_put_int(int64_t x, Sink &sink, int p) {
    uint64_t mag = x < 0 ? 0 - (uint64_t)x : (uint64_t)x;
    const int nd = mag ? tt_ndigits(mag) : 1;
    int b = p;
    if (x < 0) sink.put(b++, '-');
    for (int i = nd - 1; i >= 0; i--) {
        const uint64_t t = mag / 10;
        sink.put(b + i, (unsigned char)('0' + (int)(mag - 10 * t)));
        mag = t;
    }
    return (x < 0 ? 1 : 0) + nd;
}

// a plain buffer as a sink (the host entry points, the selftest kernel's 24-byte slots)
struct TtBufferSink {
    unsigned char *buf;
    TT_HD inline void put(int p, unsigned char c) { buf[p] = c; }
};

}  // namespace cd
