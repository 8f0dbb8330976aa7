// chinput_tile.h — what the device readers of text tables share (chinput_kernels.hip, peaks_kernels.hip): the tile constants, the
// bounds-checked byte reader, the marks of the non-blank line starts in one lane's chunk, the scan inside the workgroup, and the reader
// of a tile's lines (the staged window first, global memory behind it).  Line rule: include/chicdiff_hip.h, above
// chicdiff_hip_chinput_parse_dev.  Everything here has internal linkage: each of the two sources compiles its own copy.
#pragma once
#include "common.h"

namespace cd {

namespace {

constexpr int kChTile = CHICDIFF_CHINPUT_TILE_BYTES;
constexpr int kChLane = CHICDIFF_CHINPUT_LANE_BYTES;
constexpr int kChWindow = CHICDIFF_CHINPUT_WINDOW_BYTES;
constexpr int kChLanes = 256;
constexpr int kChMaxLines = kChTile / 2;  // a row is at least one character and its '\n': two line starts lie two bytes apart
static_assert(kChLane == 64, "a lane's marks are one 64-bit word, its chunk four 16-byte loads");
static_assert(kChTile == kChLanes * kChLane, "256 lanes, one chunk each");
static_assert(kChWindow > kChTile && kChWindow % 16 == 0 && kChTile <= 65536, "the overhang holds at least the byte after the tile; tile offsets are 16-bit");

// Bytes outside the body read as '\n': the position before the body's first byte ends a line, and the body's end ends the last one.
__device__ __forceinline__ unsigned char ch_byte(const unsigned char *__restrict__ text, int64_t n, int64_t i) {
    return (i >= 0 && i < n) ? text[i] : (unsigned char)'\n';
}

// 16 bytes at `off` (a multiple of 16; text is 16-byte aligned), '\n' beyond the body
__device__ __forceinline__ uint4 ch_load16(const unsigned char *__restrict__ text, int64_t n, int64_t off) {
    if (off + 16 <= n) return *reinterpret_cast<const uint4 *>(text + off);
    uint32_t w[4];
#pragma unroll
    for (int k = 0; k < 4; k++) {
        w[k] = 0;
#pragma unroll
        for (int b = 0; b < 4; b++) w[k] |= (uint32_t)ch_byte(text, n, off + 4 * k + b) << (8 * b);
    }
    return make_uint4(w[0], w[1], w[2], w[3]);
}

// bit k of the result: byte k of the chunk starts a line that is not blank.  prev = the byte before the chunk, next = the byte after.
__device__ __forceinline__ uint64_t ch_marks(const uint4 v[4], unsigned char prev, unsigned char next) {
    const uint32_t w[16] = {v[0].x, v[0].y, v[0].z, v[0].w, v[1].x, v[1].y, v[1].z, v[1].w,
                            v[2].x, v[2].y, v[2].z, v[2].w, v[3].x, v[3].y, v[3].z, v[3].w};
    uint64_t nl = 0, cr = 0;  // bit k: byte k is '\n' / '\r'
#pragma unroll
    for (int k = 0; k < 64; k++) {
        const uint32_t b = (w[k >> 2] >> (8 * (k & 3))) & 0xffu;
        nl |= (uint64_t)(b == '\n') << k;
        cr |= (uint64_t)(b == '\r') << k;
    }
    const uint64_t after_nl = (nl << 1) | (uint64_t)(prev == '\n');            // bit k: byte k - 1 is '\n'
    const uint64_t nl_next = (nl >> 1) | ((uint64_t)(next == '\n') << 63);     // bit k: byte k + 1 is '\n'
    return after_nl & ~nl & ~(cr & nl_next);
}

// exclusive scan of one int per lane over the workgroup's 256 lanes; *total = the sum.  s_wave: 4 ints of LDS.
__device__ __forceinline__ int ch_block_scan(int v, int *s_wave, int *total) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    int inc = v;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const int t = __shfl_up(inc, d, 64);
        if (lane >= d) inc += t;
    }
    if (lane == 63) s_wave[wave] = inc;
    __syncthreads();
    int before = 0, sum = 0;
#pragma unroll
    for (int k = 0; k < kChLanes / 64; k++) {
        const int t = s_wave[k];
        if (k < wave) before += t;
        sum += t;
    }
    *total = sum;
    return before + inc - v;
}

// the bytes of one tile's lines: the staged window first, global memory behind it
struct ChReader {
    const unsigned char *win;   // LDS, kChWindow bytes from `base` ('\n' beyond the body)
    const unsigned char *text;
    int64_t n, base;
    __device__ __forceinline__ unsigned char at(int64_t p) const {  // p: offset from the tile's first byte
        return p < kChWindow ? win[p] : ch_byte(text, n, base + p);
    }
    // the line ends at p: its '\n', the body's end, or one '\r' in front of either
    __device__ __forceinline__ bool line_end(unsigned char c, int64_t p) const { return c == '\n' || (c == '\r' && at(p + 1) == '\n'); }
};

}  // namespace

}  // namespace cd
