// ru_window.h — the window of one peak in getRegionUniverse: .expandAvoidBait(bait, oe, s) of chicdiff.R:353-367, clamped to the map.
// The rule for IDs off the map stands above chicdiff_hip_region_universe_count_dev in include/chicdiff_hip.h.
//
//   dist > s + 1   (oe - s):(oe + s)
//   oe > bait      (bait + 2):(oe + s)
//   oe < bait      (oe - s):(bait - 2)
//   oe == bait     stop("Invalid parameters")
// R's a:b counts down when a > b, so the set is [min(a, b), max(a, b)].  bait and oe are any int32 (the peak reader admits every int32
// ID), so oe + s, oe - s, bait + 2, bait - 2 and |bait - oe| do not fit 32 bits: everything is formed in 64.  Only IDs in [1, maxfrag]
// are ever kept (the rmap join, :389-391, and `otherEndID <= maxfrag`, :384), so the window is clamped to that range, which changes no
// result and bounds every loop over it by the map; an empty window comes back as lo = 1, hi = 0.
// Host and device code: post_kernels.hip runs it per region, tests/region_window_host.cpp on its own.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#define RU_HD __host__ __device__
#else
#define RU_HD
#endif

namespace cd {

// The largest maxfrag the region-universe entry points take: with the window inside [1, 2^30) a 32-bit counter that steps by four, and
// hi - lo, cannot overflow.  (chr_of alone would be 4 GiB there.)
constexpr int32_t kRuMaxFrag = (1 << 30) - 1;

// false = baitID == oeID (the reference stops); lo, hi are then the empty window too
RU_HD inline bool ru_window(int32_t bait, int32_t oe, int32_t s, int32_t maxfrag, int32_t &lo, int32_t &hi) {
    const int64_t b = bait, o = oe, w = s;
    const int64_t dist = b > o ? b - o : o - b;
    int64_t a = 1, e = 0;
    bool ok = true;
    if (dist > w + 1) { a = o - w; e = o + w; }
    else if (o > b) { a = b + 2; e = o + w; }
    else if (o < b) { a = o - w; e = b - 2; }
    else ok = false;
    int64_t l = a < e ? a : e, h = a < e ? e : a;
    if (l < 1) l = 1;
    if (h > maxfrag) h = maxfrag;
    if (!ok || l > h) { l = 1; h = 0; }
    lo = (int32_t)l;
    hi = (int32_t)h;
    return ok;
}

}  // namespace cd
