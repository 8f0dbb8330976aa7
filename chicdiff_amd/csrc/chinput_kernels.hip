// chinput_kernels.hip — f2, text part on the device: the body of a .chinput file (the bytes after its header line) -> the three int32
// columns baitID, otherEndID, N in file order.  The rule is stated above chicdiff_hip_chinput_parse_dev in include/chicdiff_hip.h and
// is the one chinput.hip's host parser follows.  gfx950 only.
//
//   which bytes start a row      -> chinput_mark_kernel: a workgroup takes one tile of kChTile consecutive bytes, a lane one chunk of
//                                   kChLane bytes with 16-byte loads; a position is counted when it is the body start or follows a
//                                   '\n' and its line is not blank (which takes the next byte and the one after).  One count per tile.
//   row number of a line         -> one exclusive scan of the tile counts (rocPRIM); the total is nrows
//   the three values of a row    -> chinput_parse_kernel: the same tile staged in LDS with an overhang (kChWindow bytes), the same
//                                   marks, a scan of the lanes' counts inside the workgroup, the line starts compacted in LDS; then
//                                   one lane parses one line and writes its three values at [tile base + rank in the tile].  A line
//                                   that runs past the staged window is continued from global memory.
//
// No value passes through an atomic: a row's place comes from the two scans alone, so launch shape and arrival order cannot show in
// the result.  The one atomic is the 64-bit minimum over the offsets of the malformed lines.  No kernel here takes a lock or polls.
#include <string.h>

#include <rocprim/rocprim.hpp>

#include "common.h"
#include "chinput_tile.h"

namespace cd {

namespace {

// ---- mark pass -------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(kChLanes) void chinput_mark_kernel(const unsigned char *__restrict__ text, int64_t n, int64_t *__restrict__ counts) {
    __shared__ int s_wave[kChLanes / 64];
    const int64_t off = (int64_t)blockIdx.x * kChTile + (int64_t)threadIdx.x * kChLane;
    int c = 0;
    if (off < n) {
        uint4 v[4];
#pragma unroll
        for (int k = 0; k < 4; k++) v[k] = ch_load16(text, n, off + 16 * k);
        c = __popcll(ch_marks(v, ch_byte(text, n, off - 1), ch_byte(text, n, off + kChLane)));
    }
    int total;
    (void)ch_block_scan(c, s_wave, &total);
    if (threadIdx.x == 0) counts[blockIdx.x] = (int64_t)total;
}

// ---- parse pass ------------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ bool ch_is_sep(unsigned char c) { return c == '\t' || c == ' ' || c == ','; }

// one line from p on: columns ib, io, in (0-based) must be integers; nothing behind the largest of them is looked at
__device__ bool ch_parse_line(const ChReader &rd, int64_t p, int ib, int io, int in, int last, int32_t out[3]) {
    int col = 0, got = 0;
    for (;;) {
        unsigned char c = rd.at(p);
        if (col == ib || col == io || col == in) {
            bool neg = false;
            if (c == '-' || c == '+') {
                neg = c == '-';
                c = rd.at(++p);
            }
            long long v = 0;
            bool digits = false;
            while (!ch_is_sep(c) && !rd.line_end(c, p)) {
                if (c < '0' || c > '9') return false;
                v = v * 10 + (c - '0');
                if (v > 2147483647LL) return false;
                digits = true;
                c = rd.at(++p);
            }
            if (!digits) return false;
            out[col == ib ? 0 : (col == io ? 1 : 2)] = (int32_t)(neg ? -v : v);
            got++;
        } else {
            while (!ch_is_sep(c) && !rd.line_end(c, p)) c = rd.at(++p);
        }
        col++;
        if (!ch_is_sep(c) || col > last) break;  // the line's end, or every needed column seen
        p++;
        if (rd.line_end(rd.at(p), p)) break;     // a separator as the line's last character opens no further field
    }
    return got == 3;
}

__global__ __launch_bounds__(kChLanes) void chinput_parse_kernel(const unsigned char *__restrict__ text, int64_t n, const int64_t *__restrict__ tile_row,
                                                                 int ib, int io, int in, int32_t *__restrict__ bait, int32_t *__restrict__ oe,
                                                                 int32_t *__restrict__ N, int64_t cap, unsigned long long *bad) {
    __shared__ uint4 s_win4[kChWindow / 16];
    __shared__ unsigned short s_start[kChMaxLines];
    __shared__ int s_wave[kChLanes / 64];
    unsigned char *s_win = reinterpret_cast<unsigned char *>(s_win4);
    const int64_t base = (int64_t)blockIdx.x * kChTile;
    for (int j = threadIdx.x; j < kChWindow / 16; j += kChLanes) s_win4[j] = ch_load16(text, n, base + 16 * (int64_t)j);
    __syncthreads();
    // the marks of this lane's chunk, from the staged bytes
    const int o = threadIdx.x * kChLane;
    uint4 v[4];
#pragma unroll
    for (int k = 0; k < 4; k++) v[k] = s_win4[threadIdx.x * (kChLane / 16) + k];
    uint64_t m = ch_marks(v, o > 0 ? s_win[o - 1] : ch_byte(text, n, base - 1), s_win[o + kChLane]);
    int nlines;
    int r = ch_block_scan(__popcll(m), s_wave, &nlines);
    while (m) {  // compact the line starts, in position order
        const int k = __ffsll((unsigned long long)m) - 1;
        m &= m - 1;
        s_start[r++] = (unsigned short)(o + k);
    }
    __syncthreads();
    ChReader rd;
    rd.win = s_win; rd.text = text; rd.n = n; rd.base = base;
    const int last = ib > io ? (ib > in ? ib : in) : (io > in ? io : in);
    const int64_t row0 = tile_row[blockIdx.x];
    for (int i = threadIdx.x; i < nlines; i += kChLanes) {
        const int64_t p = s_start[i], row = row0 + i;
        int32_t val[3];
        if (!ch_parse_line(rd, p, ib, io, in, last, val)) {
            atomicMin(bad, (unsigned long long)(base + p));
        } else if (row < cap) {
            bait[row] = val[0];
            oe[row] = val[1];
            N[row] = val[2];
        }
    }
}

size_t ch_c256(size_t x) { return (x + 255) & ~(size_t)255; }

int64_t ch_tiles(int64_t nbytes) { return (nbytes + kChTile - 1) / kChTile; }

size_t ch_scan_bytes(int64_t ntiles) {
    size_t b = 0;
    int64_t *d = nullptr;
    (void)rocprim::exclusive_scan(nullptr, b, d, d, (int64_t)0, (size_t)ntiles + 1, rocprim::plus<int64_t>(), (hipStream_t)0);
    return b + 256;
}

}  // namespace

size_t chinput_workspace_bytes(int64_t nbytes) {
    const int64_t ntiles = ch_tiles(nbytes);
    return 256 + ch_c256(sizeof(int64_t) * (size_t)(ntiles + 1)) + ch_scan_bytes(ntiles);
}

// mark pass + scan, enqueued on `st`; *nrows_out / *bad_out are device words inside ws: the row count (valid once the stream has run),
// and the word the parse pass takes the minimum into (all ones = no malformed line)
int launch_chinput_count(const unsigned char *text, int64_t nbytes, char *ws, hipStream_t st, const int64_t **nrows_out,
                         const unsigned long long **bad_out) {
    const int64_t ntiles = ch_tiles(nbytes);
    unsigned long long *bad = (unsigned long long *)ws;
    int64_t *counts = (int64_t *)(ws + 256);
    *nrows_out = counts + ntiles;
    *bad_out = bad;
    if (hipMemsetAsync(bad, 0xff, sizeof(unsigned long long), st) != hipSuccess) return 1;
    if (hipMemsetAsync(counts + ntiles, 0, sizeof(int64_t), st) != hipSuccess) return 1;
    chinput_mark_kernel<<<(unsigned)ntiles, kChLanes, 0, st>>>(text, nbytes, counts);
    return 0;
}
int launch_chinput_scan(int64_t nbytes, char *ws, hipStream_t st) {
    const int64_t ntiles = ch_tiles(nbytes);
    int64_t *counts = (int64_t *)(ws + 256);
    void *tmp = ws + 256 + ch_c256(sizeof(int64_t) * (size_t)(ntiles + 1));
    size_t tmp_bytes = ch_scan_bytes(ntiles);
    return rocprim::exclusive_scan(tmp, tmp_bytes, counts, counts, (int64_t)0, (size_t)ntiles + 1, rocprim::plus<int64_t>(), st) == hipSuccess ? 0 : 1;
}
// parse pass, after launch_chinput_count + launch_chinput_scan on the same ws
void launch_chinput_parse(const unsigned char *text, int64_t nbytes, int ib, int io, int in, int32_t *bait, int32_t *oe, int32_t *N, int64_t cap,
                          char *ws, hipStream_t st) {
    chinput_parse_kernel<<<(unsigned)ch_tiles(nbytes), kChLanes, 0, st>>>(text, nbytes, (const int64_t *)(ws + 256), ib, io, in, bait, oe, N, cap,
                                                                        (unsigned long long *)ws);
}

}  // namespace cd
