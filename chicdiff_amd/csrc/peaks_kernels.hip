// peaks_kernels.hip — readAndFilterPeakMatrix on the device (chicdiff.R:218-277): the body of a peak matrix (the bytes after its header
// line) -> six int32 columns, dist, the score matrix and every row's line offset, in file order; then the four filters, the kept rows
// compacted in file order and the baits left without a kept row in order of first appearance.  The rule is stated above
// chicdiff_hip_peaks_parse_dev in include/chicdiff_hip.h.  gfx950 only.
//
//   lines                        -> the mark pass and the scan of chinput_kernels.hip, unchanged (launch_chinput_count / _scan)
//   a '"' anywhere in the body   -> peaks_quote_kernel, before the first host stop: such a body is not parsed here
//   the values of a row          -> peaks_parse_kernel: tile, window and compaction of chinput_parse_kernel (chinput_tile.h); one lane
//                                   parses one line; decimal fields through peaks_decimal.h, exact; a token outside its domain goes on
//                                   a bounded list (one counter; each cell is patched independently, so the slot order cannot show)
//   keep / drop                  -> peaks_filter_kernel: the predicate per row; per bait a 64-bit minimum over (kept ? row : row + 2^62):
//                                   below 2^62 once the bait has a kept row, else its first row
//   places                       -> peaks_bait_flag_kernel marks the first row of every bait without a kept row; ONE exclusive scan
//                                   (rocPRIM) of the packed flags (kept in the low half, such a first row in the high half);
//                                   peaks_compact_kernel writes both lists.  Both come out in file order with no sort.
//
// No value passes through an atomic: the atomics are the two 64-bit minima (malformed offset, the bait table), the maximum of baitID and
// the slow list's counter.  No kernel here takes a lock or polls.
#include <stddef.h>
#include <string.h>

#include <rocprim/rocprim.hpp>

#include "chinput_tile.h"
#include "common.h"
#include "peaks.h"
#include "peaks_decimal.h"

namespace cd {

namespace {

constexpr unsigned long long kPkNotKept = 1ull << 62;

// ---- quote pass ------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(kChLanes) void peaks_quote_kernel(const unsigned char *__restrict__ text, int64_t n, PeaksCounters *__restrict__ cnt) {
    const int64_t off = (int64_t)blockIdx.x * kChTile + (int64_t)threadIdx.x * kChLane;
    if (off >= n) return;
    bool q = false;
#pragma unroll
    for (int k = 0; k < 4; k++) {
        const uint4 v = ch_load16(text, n, off + 16 * k);
        const uint32_t w[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
        for (int j = 0; j < 4; j++) {
            const uint32_t x = w[j] ^ 0x22222222u;  // a zero byte where the text holds '"'
            q = q || (((x - 0x01010101u) & ~x & 0x80808080u) != 0);
        }
    }
    if (q) cnt->quote = 1;  // (every writer stores the same value)
}

// ---- parse pass ------------------------------------------------------------------------------------------------------------------
// what a field of the first eleven is: 0 text, 1 .. 6 the int32 column (1-based), 7 dist
__device__ __forceinline__ int pk_key_kind(int col) {
    switch (col) {
        case 1: return 1;   // baitStart
        case 2: return 2;   // baitEnd
        case 3: return 3;   // baitID
        case 6: return 4;   // oeStart
        case 7: return 5;   // oeEnd
        case 8: return 6;   // oeID
        case 10: return 7;  // dist
        default: return 0;
    }
}

// one line from p on.  false = malformed.  Scores and slow-list entries are written as they are met (row < cap only); the seven key
// values come back in iv / dist.
__device__ bool pk_parse_line(const ChReader &rd, int64_t p, unsigned char sep, const int *s_col, int nscore, int last,
                              const uint64_t (*pow5)[2], int64_t row, const PeaksOut &o, PeaksCounters *cnt, PeaksSlow *slow_list,
                              int32_t iv[6], double *dist) {
    int col = 0, j = 0;
    for (;;) {
        unsigned char c = rd.at(p);
        int kind = 0;
        if (col < CHICDIFF_PEAKS_KEY_COLUMNS) kind = pk_key_kind(col);
        else if (j < nscore && col == s_col[j]) kind = 8;
        if (kind >= 1 && kind <= 6) {  // chinput's integer rule
            bool neg = false;
            if (c == '-' || c == '+') {
                neg = c == '-';
                c = rd.at(++p);
            }
            long long v = 0;
            bool digits = false;
            while (c != sep && !rd.line_end(c, p)) {
                if (c < '0' || c > '9') return false;
                v = v * 10 + (c - '0');
                if (v > 2147483647LL) return false;
                digits = true;
                c = rd.at(++p);
            }
            if (!digits) return false;
            if (neg) v = -v;
            if ((kind == 3 || kind == 6) && v < 0) return false;  // baitID, oeID
            iv[kind - 1] = (int32_t)v;
        } else if (kind >= 7) {
            const int64_t start = p;
            double v;
            const int rc = pk_scan_decimal(rd, p, sep, pow5, &v);
            if (rc == PK_MALFORMED) return false;
            c = rd.at(p);
            if (rc == PK_SLOW && row < o.cap) {
                const unsigned int slot = atomicAdd(&cnt->nslow, 1u);
                if (slot < (unsigned int)CHICDIFF_PEAKS_MAX_SLOW) {
                    slow_list[slot].row = row;
                    slow_list[slot].col = kind == 7 ? -1 : j;
                    slow_list[slot].off = rd.base + start;
                }
            }
            if (kind == 7) {
                *dist = v;
            } else {
                if (row < o.cap) o.scores[(int64_t)j * o.stride + row] = v;
                j++;
            }
        } else {
            while (c != sep && !rd.line_end(c, p)) c = rd.at(++p);
        }
        if (col == last) return true;  // every needed column seen: nothing behind it is looked at
        if (c != sep) return false;    // the line ends with fields missing
        col++;
        p++;
    }
}

__global__ __launch_bounds__(kChLanes) void peaks_parse_kernel(const unsigned char *__restrict__ text, int64_t n, const int64_t *__restrict__ tile_row,
                                                               int sep, const int *__restrict__ score_cols, int nscore, PeaksOut o,
                                                               unsigned long long *bad, PeaksCounters *cnt, PeaksSlow *slow_list) {
    __shared__ uint4 s_win4[kChWindow / 16];
    __shared__ unsigned short s_start[kChMaxLines];
    __shared__ int s_wave[kChLanes / 64];
    __shared__ uint64_t s_pow5[kPow5Max + 1][2];
    __shared__ int s_col[CHICDIFF_PEAKS_MAX_SCORES];
    unsigned char *s_win = reinterpret_cast<unsigned char *>(s_win4);
    const int64_t base = (int64_t)blockIdx.x * kChTile;
    for (int j = threadIdx.x; j < kChWindow / 16; j += kChLanes) s_win4[j] = ch_load16(text, n, base + 16 * (int64_t)j);
    for (int j = threadIdx.x; j < 2 * (kPow5Max + 1); j += kChLanes) s_pow5[j >> 1][j & 1] = kPow5[j >> 1][j & 1];
    for (int j = threadIdx.x; j < CHICDIFF_PEAKS_MAX_SCORES; j += kChLanes) s_col[j] = j < nscore ? score_cols[j] : 0x7fffffff;
    __syncthreads();
    // the marks of this lane's chunk, from the staged bytes
    const int oc = threadIdx.x * kChLane;
    uint4 v[4];
#pragma unroll
    for (int k = 0; k < 4; k++) v[k] = s_win4[threadIdx.x * (kChLane / 16) + k];
    uint64_t m = ch_marks(v, oc > 0 ? s_win[oc - 1] : ch_byte(text, n, base - 1), s_win[oc + kChLane]);
    int nlines;
    int r = ch_block_scan(__popcll(m), s_wave, &nlines);
    while (m) {  // compact the line starts, in position order
        const int k = __ffsll((unsigned long long)m) - 1;
        m &= m - 1;
        s_start[r++] = (unsigned short)(oc + k);
    }
    __syncthreads();
    ChReader rd;
    rd.win = s_win; rd.text = text; rd.n = n; rd.base = base;
    const int last = nscore > 0 ? s_col[nscore - 1] : CHICDIFF_PEAKS_KEY_COLUMNS - 1;
    const int64_t row0 = tile_row[blockIdx.x];
    int maxbait = -1;
    for (int i = threadIdx.x; i < nlines; i += kChLanes) {
        const int64_t p = s_start[i], row = row0 + i;
        int32_t iv[6];
        double dist;
        if (!pk_parse_line(rd, p, (unsigned char)sep, s_col, nscore, last, s_pow5, row, o, cnt, slow_list, iv, &dist)) {
            atomicMin(bad, (unsigned long long)(base + p));
        } else if (row < o.cap) {
#pragma unroll
            for (int k = 0; k < 6; k++) o.ints[(int64_t)k * o.stride + row] = iv[k];
            o.dist[row] = dist;
            o.line_off[row] = base + p;
            maxbait = iv[2] > maxbait ? iv[2] : maxbait;
        }
    }
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) {
        const int t = __shfl_xor(maxbait, d, 64);
        maxbait = t > maxbait ? t : maxbait;
    }
    if ((threadIdx.x & 63) == 0 && maxbait >= 0) atomicMax(&cnt->maxbait, maxbait);
}

// one cell per slow token, from the host's strtod
__global__ void peaks_patch_kernel(const PeaksSlow *__restrict__ list, const double *__restrict__ val, int nslow, PeaksOut o) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= nslow) return;
    const int64_t row = list[i].row, col = list[i].col;
    if (row < 0 || row >= o.cap) return;
    if (col < 0) o.dist[row] = val[i];
    else o.scores[col * o.stride + row] = val[i];
}

// ---- filter ----------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void peaks_filter_kernel(const int32_t *__restrict__ bait, const int32_t *__restrict__ oe,
                                                           const double *__restrict__ dist, const double *__restrict__ scores, int64_t stride,
                                                           int64_t n, int nscore, double score, const int *__restrict__ cond_of_col, int ncond,
                                                           int replicate_rule, int64_t maxbait, unsigned long long *__restrict__ table,
                                                           int64_t *__restrict__ flags) {
    __shared__ int s_cond[CHICDIFF_PEAKS_MAX_SCORES];
    for (int j = threadIdx.x; j < nscore; j += blockDim.x) s_cond[j] = cond_of_col[j];
    __syncthreads();
    const int64_t r = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (r > n) return;
    if (r == n) {  // the scan's last entry: the totals land here
        flags[n] = 0;
        return;
    }
    bool keep = false;
    for (int j = 0; j < nscore; j++) keep = keep || scores[(int64_t)j * stride + r] > score;  // NaN never passes
    if (keep && replicate_rule) {
        for (int c = 0; c < ncond && keep; c++) {
            int cntc = 0;
            for (int j = 0; j < nscore; j++) {
                const double s = scores[(int64_t)j * stride + r];
                cntc += (s_cond[j] == c) && (s == s);
            }
            keep = cntc >= 2;
        }
    }
    const int64_t b = bait[r], o = oe[r];
    keep = keep && dist[r] == dist[r] && o != b + 1 && o != b - 1;
    flags[r] = keep ? 1 : 0;
    if (b >= 0 && b <= maxbait) atomicMin(&table[b], (unsigned long long)r | (keep ? 0ull : kPkNotKept));
}

__global__ __launch_bounds__(256) void peaks_bait_flag_kernel(const int32_t *__restrict__ bait, int64_t n, int64_t maxbait,
                                                              const unsigned long long *__restrict__ table, int64_t *__restrict__ flags) {
    const int64_t r = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (r >= n) return;
    const int64_t b = bait[r];
    if (flags[r] == 0 && b >= 0 && b <= maxbait && table[b] == ((unsigned long long)r | kPkNotKept)) flags[r] = 1ll << 32;
}

__global__ __launch_bounds__(256) void peaks_compact_kernel(const int32_t *__restrict__ bait, const int32_t *__restrict__ oe, int64_t n,
                                                            const int64_t *__restrict__ pos, int64_t *__restrict__ kept_idx,
                                                            int32_t *__restrict__ kept_bait, int32_t *__restrict__ kept_oe,
                                                            int32_t *__restrict__ filtered) {
    const int64_t r = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (r >= n) return;
    const int64_t at = pos[r], d = pos[r + 1] - at;
    if (d & 1) {
        const int64_t k = at & 0xffffffffll;
        if (k < n) {
            kept_idx[k] = r;
            kept_bait[k] = bait[r];
            kept_oe[k] = oe[r];
        }
    } else if (d >> 32) {
        const int64_t k = at >> 32;
        if (k < n) filtered[k] = bait[r];
    }
}

size_t pk_c256(size_t x) { return (x + 255) & ~(size_t)255; }

size_t pk_scan_bytes(int64_t n) {
    size_t b = 0;
    int64_t *d = nullptr;
    (void)rocprim::exclusive_scan(nullptr, b, d, d, (int64_t)0, (size_t)n + 1, rocprim::plus<int64_t>(), (hipStream_t)0);
    return pk_c256(b) + 256;  // a multiple of 256: the bait table's 64-bit words lie behind it
}

}  // namespace

// ---- parse: workspace = [chinput's workspace][counters 256][score columns 256][slow list] ------------------------------------------------
static size_t pk_parse_base(int64_t nbytes) { return pk_c256(chinput_workspace_bytes(nbytes)); }
size_t peaks_parse_workspace_bytes(int64_t nbytes) {
    return pk_parse_base(nbytes) + 256 + 256 + pk_c256(sizeof(PeaksSlow) * (size_t)CHICDIFF_PEAKS_MAX_SLOW);
}
PeaksCounters *peaks_counters(char *ws, int64_t nbytes) { return (PeaksCounters *)(ws + pk_parse_base(nbytes)); }
PeaksSlow *peaks_slow_list(char *ws, int64_t nbytes) { return (PeaksSlow *)(ws + pk_parse_base(nbytes) + 512); }

// before the first host stop, after launch_chinput_count on the same ws: the counters cleared, the score columns up, the quote pass
int launch_peaks_prepare(const unsigned char *text, int64_t nbytes, const int32_t *score_cols_host, int nscore, char *ws, hipStream_t st) {
    PeaksCounters *cnt = peaks_counters(ws, nbytes);
    static_assert(sizeof(PeaksCounters) <= 256 && offsetof(PeaksCounters, maxbait) == 0, "the counters have a 256-byte slot, maxbait first");
    if (hipMemsetAsync(cnt, 0, 256, st) != hipSuccess) return 1;
    if (hipMemsetAsync(cnt, 0xff, sizeof(int), st) != hipSuccess) return 1;  // maxbait = -1: no row yet
    if (nscore > 0 && hipMemcpyAsync(ws + pk_parse_base(nbytes) + 256, score_cols_host, sizeof(int32_t) * (size_t)nscore, hipMemcpyHostToDevice, st) != hipSuccess)
        return 1;
    const int64_t ntiles = (nbytes + kChTile - 1) / kChTile;
    peaks_quote_kernel<<<(unsigned)ntiles, kChLanes, 0, st>>>(text, nbytes, cnt);
    return 0;
}

// parse pass, after launch_chinput_count + launch_chinput_scan + launch_peaks_prepare on the same ws
void launch_peaks_parse(const unsigned char *text, int64_t nbytes, int sep, int nscore, const PeaksOut &o, char *ws, hipStream_t st) {
    const int64_t ntiles = (nbytes + kChTile - 1) / kChTile;
    peaks_parse_kernel<<<(unsigned)ntiles, kChLanes, 0, st>>>(text, nbytes, (const int64_t *)(ws + 256), sep, (const int *)(ws + pk_parse_base(nbytes) + 256),
                                                            nscore, o, (unsigned long long *)ws, peaks_counters(ws, nbytes),
                                                            peaks_slow_list(ws, nbytes));
}

// d_val: nslow doubles in device memory, in the slow list's order
void launch_peaks_patch(const double *d_val, int nslow, const PeaksOut &o, char *ws, int64_t nbytes, hipStream_t st) {
    if (nslow <= 0) return;
    peaks_patch_kernel<<<(unsigned)((nslow + 255) / 256), 256, 0, st>>>(peaks_slow_list(ws, nbytes), d_val, nslow, o);
}

// ---- filter: workspace = [cond_of_col 256][flags (n + 1)][scan temporaries][bait table (maxbait + 1)] -----------------------------------
size_t peaks_filter_workspace_bytes(int64_t n, int64_t maxbait) {
    return 256 + pk_c256(sizeof(int64_t) * (size_t)(n + 1)) + pk_scan_bytes(n) + pk_c256(sizeof(unsigned long long) * (size_t)(maxbait + 1));
}

// *totals_out: a device word, kept rows in its low half and baits without a kept row in its high half, valid once the stream has run
int launch_peaks_filter(const int32_t *bait, const int32_t *oe, const double *dist, const double *scores, int64_t stride, int64_t n, int nscore,
                        double score, const int32_t *cond_of_col_host, int ncond, int replicate_rule, int64_t maxbait, int64_t *kept_idx,
                        int32_t *kept_bait, int32_t *kept_oe, int32_t *filtered, char *ws, hipStream_t st, const int64_t **totals_out) {
    int *d_cond = (int *)ws;
    int64_t *flags = (int64_t *)(ws + 256);
    void *tmp = ws + 256 + pk_c256(sizeof(int64_t) * (size_t)(n + 1));
    size_t tmp_bytes = pk_scan_bytes(n);
    unsigned long long *table = (unsigned long long *)((char *)tmp + tmp_bytes);
    *totals_out = flags + n;
    if (nscore > 0 && hipMemcpyAsync(d_cond, cond_of_col_host, sizeof(int32_t) * (size_t)nscore, hipMemcpyHostToDevice, st) != hipSuccess) return 1;
    if (maxbait >= 0 && hipMemsetAsync(table, 0xff, sizeof(unsigned long long) * (size_t)(maxbait + 1), st) != hipSuccess) return 1;
    const unsigned blocks = (unsigned)((n + 1 + 255) / 256);
    peaks_filter_kernel<<<blocks, 256, 0, st>>>(bait, oe, dist, scores, stride, n, nscore, score, d_cond, ncond, replicate_rule, maxbait, table, flags);
    peaks_bait_flag_kernel<<<blocks, 256, 0, st>>>(bait, n, maxbait, table, flags);
    if (rocprim::exclusive_scan(tmp, tmp_bytes, flags, flags, (int64_t)0, (size_t)n + 1, rocprim::plus<int64_t>(), st) != hipSuccess) return 1;
    peaks_compact_kernel<<<blocks, 256, 0, st>>>(bait, oe, n, flags, kept_idx, kept_bait, kept_oe, filtered);
    return 0;
}

}  // namespace cd
