// global_kernels.hip — exact medians over all rows.
//
//  * exact medians (size factors, chicdiff.R:1561-1562 / A1; MAD of log residuals, A3) by a
//    12-bit radix select over order-preserving 64-bit keys: two histogram rounds, then the few
//    hundred candidates left are gathered and sorted (single rank: compaction; sharded: count rows
//    + a sum-all-reduce of disjoint entries) — every step is a SUM, so it shards;
//  * the direct route to the size factors: two passes over the counts and a value-binned select,
//    the keys never stored (sf_*; the bin function is in common.h).
#include "common.h"
#include "devmath.h"
#include "prior_mc.h"

namespace cd {

// ------------------------------------------------------------------------------------------
// radix select
__device__ __forceinline__ bool sel_key(const SelArgs &a, const FitScalars *sc, int col, int64_t i, uint64_t &key) {
    double x;
    if (a.mode == SEL_SIZEFACTOR) {
        x = a.ratio[(int64_t)col * a.n + i];  // log(k) - loggeomean, NaN = excluded (row_ratio_kernel)
        if (x != x) return false;
    } else {
        x = a.resid[i];
        if (x != x) return false;
        if (a.mode == SEL_ABSDEV) x = fabs(x - sc->med);
    }
    key = key_of(x);
    return true;
}

// the element behind sel_key() as it sits in memory (NaN = excluded), and the key of a loaded element: the row loops below load
// four elements before they work on the first, so that a thread has four loads in flight instead of one
__device__ __forceinline__ double sel_raw(const SelArgs &a, int col, int64_t i) {
    return a.mode == SEL_SIZEFACTOR ? a.ratio[(int64_t)col * a.n + i] : a.resid[i];
}
__device__ __forceinline__ bool sel_key_of_raw(const SelArgs &a, const FitScalars *sc, double x, uint64_t &key) {
    if (x != x) return false;
    if (a.mode == SEL_ABSDEV) x = fabs(x - sc->med);
    key = key_of(x);
    return true;
}

// histograms of the current digit for the two live prefixes of column blockIdx.y
__global__ __launch_bounds__(256) void sel_hist_kernel(SelArgs a, FitWork w, int bits) {
    __shared__ unsigned int h[2][kSelBins];
    const int col = blockIdx.y;
    const FitScalars *sc = w.sc;
    if (!sel_first_round(a.shift) && sc->sel_fast_done) return;  // the shortcut already has the answers
    for (int k = threadIdx.x; k < 2 * kSelBins; k += 256) (&h[0][0])[k] = 0;
    __syncthreads();
    const bool first = sel_first_round(a.shift);  // first round: every key, whatever an earlier select left behind
    const uint64_t p0 = first ? 0 : sc->sel_prefix[2 * col], p1 = first ? 0 : sc->sel_prefix[2 * col + 1];
    const int hi = a.shift + bits;  // bits above `hi` are fixed by the prefix
    const bool same = (p0 == p1);
    const uint64_t mask = (1ull << bits) - 1ull;
    uint64_t key;
    // Run-length accumulation per thread: the first digit is the sign and exponent of the key, which a whole column
    // shares but for a handful of values — 64 lanes adding 1 to the same LDS word serialise, so a thread adds a run of
    // equal digits at once (order-free sums: the histogram is the same).
    int cur = -1;
    unsigned cnt = 0;
    const int64_t step = (int64_t)gridDim.x * 256;
    for (int64_t i0 = blockIdx.x * 256 + threadIdx.x; i0 < a.n; i0 += 4 * step) {
        double x[4];
#pragma unroll
        for (int u = 0; u < 4; u++) x[u] = i0 + u * step < a.n ? sel_raw(a, col, i0 + u * step) : NAN;
#pragma unroll
        for (int u = 0; u < 4; u++) {  // (a thread's elements in the order of the one-by-one loop: the same runs)
            if (!sel_key_of_raw(a, sc, x[u], key)) continue;
            const unsigned dig = (unsigned)((key >> a.shift) & mask);
            int bin;
            if (sel_match(key, p0, hi)) bin = (int)dig;
            else if (!same && sel_match(key, p1, hi)) bin = (int)(kSelBins + dig);
            else continue;
            if (bin == cur) cnt++;
            else {
                if (cnt) atomicAdd(&(&h[0][0])[cur], cnt);
                cur = bin;
                cnt = 1;
            }
        }
    }
    if (cnt) atomicAdd(&(&h[0][0])[cur], cnt);
    __syncthreads();
    double *g = w.hist + (size_t)col * 2 * kSelBins;
    for (int k = threadIdx.x; k < 2 * kSelBins; k += 256) {
        const unsigned c = (&h[0][0])[k];
        if (c) atomicAdd(&g[k], (double)c);
    }
}

// pick the bin holding the wanted rank (parallel form of fit_state.h sel_pick); one block per
// column, both rank slots in turn: per-thread partial sums, block scan, the owning thread refines
__global__ __launch_bounds__(256) void sel_step_kernel(SelArgs a, FitWork w, int bits) {
    __shared__ double scan[256];
    const int col = blockIdx.x;
    FitScalars *sc = w.sc;
    const bool first = sel_first_round(a.shift);
    if (!first && sc->sel_fast_done) return;
    if (first && col == 0 && threadIdx.x == 0) sc->sel_fast_done = 0;  // (read again only after later launches)
    if (a.shift == 40 && threadIdx.x < 2) sc->sel_cnt[2 * col + threadIdx.x] = 0;  // write positions of the compaction that follows
    const uint64_t p0 = first ? 0 : sc->sel_prefix[2 * col], p1 = first ? 0 : sc->sel_prefix[2 * col + 1];
    double rank0 = sc->sel_rank[2 * col], rank1 = sc->sel_rank[2 * col + 1];
    const int nb = 1 << bits, per = (nb + 255) / 256;
    for (int slot = 0; slot < 2; slot++) {
        const int hslot = (slot == 1 && p0 != p1) ? 1 : 0;
        const double *g = w.hist + ((size_t)col * 2 + hslot) * kSelBins;
        double mine[16];
        double acc = 0;
#pragma unroll
        for (int k = 0; k < 16; k++) {
            const int b = threadIdx.x * per + k;
            mine[k] = (k < per && b < nb) ? g[b] : 0.0;
            acc += mine[k];
        }
        __syncthreads();
        scan[threadIdx.x] = acc;
        __syncthreads();
        for (int off = 1; off < 256; off <<= 1) {  // inclusive Hillis-Steele scan (counts: exact in fp64)
            const double add = (int)threadIdx.x >= off ? scan[threadIdx.x - off] : 0.0;
            __syncthreads();
            scan[threadIdx.x] += add;
            __syncthreads();
        }
        if (first && slot == 0) {  // the first histogram's total is the population: ranks of the two middles
            const int64_t mi = (int64_t)scan[255];
            rank0 = (double)((mi - 1) / 2);
            rank1 = (double)(mi / 2);
            if (threadIdx.x == 0) sc->sel_count[col] = (double)mi;
        }
        const double rank = slot ? rank1 : rank0;
        const double incl = scan[threadIdx.x], before = incl - acc;
        const bool last_thread = (int)threadIdx.x == (nb - 1) / per;
        if ((before <= rank && rank < incl) || (last_thread && rank >= incl && incl == scan[255])) {
            double cum = before;
            int k = 0;
            for (; k < per - 1 && threadIdx.x * per + k < nb - 1; k++) {
                if (cum + mine[k] > rank) break;
                cum += mine[k];
            }
            const int b = threadIdx.x * per + k;
            const uint64_t pre = (slot == 0) ? p0 : p1;
            sc->sel_prefix[2 * col + slot] = pre | ((uint64_t)b << a.shift);
            sc->sel_rank[2 * col + slot] = rank - cum;
        }
    }
}

// ---- single-rank shortcut: after two rounds (24 of 64 key bits fixed) only a handful of keys share
// the live prefixes; gather them and finish in one block per column instead of four more passes over
// all the data.  Exact and order-independent (a sort), so results equal the six-round path bit for bit.
__global__ __launch_bounds__(256) void sel_compact_kernel(SelArgs a, FitWork w) {
    const int col = blockIdx.y;
    FitScalars *sc = w.sc;
    const uint64_t p0 = sc->sel_prefix[2 * col], p1 = sc->sel_prefix[2 * col + 1];
    const bool same = p0 == p1;
    uint64_t *cand = reinterpret_cast<uint64_t *>(w.hist) + (size_t)col * 2 * kSelCap;
    uint64_t key;
    const int64_t step = (int64_t)gridDim.x * 256;
    for (int64_t i0 = blockIdx.x * 256 + threadIdx.x; i0 < a.n; i0 += 4 * step) {
        double x[4];
#pragma unroll
        for (int u = 0; u < 4; u++) x[u] = i0 + u * step < a.n ? sel_raw(a, col, i0 + u * step) : NAN;
#pragma unroll
        for (int u = 0; u < 4; u++) {
            if (!sel_key_of_raw(a, sc, x[u], key)) continue;
            int slot = -1;
            if (sel_match(key, p0, 40)) slot = 0;
            else if (!same && sel_match(key, p1, 40)) slot = 1;
            if (slot < 0) continue;
            const unsigned pos = atomicAdd(&sc->sel_cnt[2 * col + slot], 1u);
            if (pos < (unsigned)kSelCap) cand[(size_t)slot * kSelCap + pos] = key;
        }
    }
}
__device__ __forceinline__ void sel_tail_rounds(const SelArgs &a, FitScalars *sc, int col, unsigned int *h);
__device__ __forceinline__ void sel_finish_col(const SelArgs &a, FitScalars *sc, int c);
__global__ __launch_bounds__(256) void sel_small_kernel(SelArgs a, FitWork w) {
    __shared__ uint64_t s_k[kSelCap];
    FitScalars *sc = w.sc;
    bool fits = true;
    for (int q = 0; q < 2 * a.ncol; q++) fits &= sc->sel_cnt[q] <= (unsigned)kSelCap;  // same verdict in every block
    const int col = blockIdx.x;
    if (!fits) {  // massive ties: this column's remaining radix rounds, here and now
        sel_tail_rounds(a, sc, col, reinterpret_cast<unsigned int *>(s_k));
        if (threadIdx.x == 0) sel_finish_col(a, sc, col);
        return;
    }
    const uint64_t p0 = sc->sel_prefix[2 * col], p1 = sc->sel_prefix[2 * col + 1];
    const uint64_t *cand = reinterpret_cast<const uint64_t *>(w.hist) + (size_t)col * 2 * kSelCap;
    uint64_t result[2] = {p0, p1};
    for (int slot = 0; slot < 2; slot++) {
        const int hslot = (slot == 1 && p0 != p1) ? 1 : 0;
        const int m = (int)sc->sel_cnt[2 * col + hslot];
        if (m == 0) continue;  // empty population: prefixes stay as they are (median NaN via sel_count)
        int len = 64;
        while (len < m) len <<= 1;
        __syncthreads();
        for (int e = threadIdx.x; e < len; e += 256) s_k[e] = e < m ? cand[(size_t)hslot * kSelCap + e] : ~0ull;
        __syncthreads();
        for (int k = 2; k <= len; k <<= 1)  // bitonic sort, ascending
            for (int j = k >> 1; j > 0; j >>= 1) {
                for (int e = threadIdx.x; e < len; e += 256) {
                    const int p = e ^ j;
                    if (p > e) {
                        const uint64_t x = s_k[e], y = s_k[p];
                        const bool up = (e & k) == 0;
                        if ((x > y) == up) { s_k[e] = y; s_k[p] = x; }
                    }
                }
                __syncthreads();
            }
        const int r = (int)sc->sel_rank[2 * col + slot];  // rank inside the prefix (set by the second round)
        result[slot] = s_k[r < m ? r : m - 1];
        __syncthreads();
    }
    if (threadIdx.x == 0) {
        sc->sel_prefix[2 * col] = result[0];
        sc->sel_prefix[2 * col + 1] = result[1];
        if (col == 0) sc->sel_fast_done = 1;
        sel_finish_col(a, sc, col);  // (a column's order statistics and what follows from them are its own)
    }
}

// The shortcut's own fallback: more than kSelCap candidates share 24 key bits with a median (massive ties).
// The column's workgroup runs the four remaining radix rounds by itself — slow (one workgroup scans all n), but it
// keeps the host from launching those rounds every time just in case.  `h` : 2 x kSelBins counters in LDS.
__device__ __forceinline__ void sel_tail_rounds(const SelArgs &a, FitScalars *sc, int col, unsigned int *h) {
    __shared__ uint64_t s_pre[2];
    __shared__ double s_rank[2];
    const int nthr = blockDim.x;
    if (threadIdx.x < 2) {
        s_pre[threadIdx.x] = sc->sel_prefix[2 * col + threadIdx.x];
        s_rank[threadIdx.x] = sc->sel_rank[2 * col + threadIdx.x];
    }
    for (int r = 2; r < 6; r++) {
        const int shift = kSelShifts[r], bits = sel_bits(shift), hi = shift + bits;
        __syncthreads();
        for (int k = threadIdx.x; k < 2 * kSelBins; k += nthr) h[k] = 0;
        __syncthreads();
        const uint64_t p0 = s_pre[0], p1 = s_pre[1], mask = (1ull << bits) - 1ull;
        const bool same = p0 == p1;
        uint64_t key;
        for (int64_t i = threadIdx.x; i < a.n; i += nthr) {
            if (!sel_key(a, sc, col, i, key)) continue;
            const unsigned dig = (unsigned)((key >> shift) & mask);
            if (sel_match(key, p0, hi)) atomicAdd(&h[dig], 1u);
            else if (!same && sel_match(key, p1, hi)) atomicAdd(&h[kSelBins + dig], 1u);
        }
        __syncthreads();
        if (threadIdx.x < 2) {  // fit_state.h sel_pick, on the workgroup's own histogram
            const int slot = threadIdx.x, hslot = (slot == 1 && !same) ? 1 : 0;
            const double rank = s_rank[slot];
            const int nb = 1 << bits;
            double cum = 0;
            int b = 0;
            for (; b < nb - 1; b++) {
                if (cum + (double)h[hslot * kSelBins + b] > rank) break;
                cum += (double)h[hslot * kSelBins + b];
            }
            s_pre[slot] = (slot ? p1 : p0) | ((uint64_t)b << shift);
            s_rank[slot] = rank - cum;
        }
        __syncthreads();
    }
    if (threadIdx.x < 2) sc->sel_prefix[2 * col + threadIdx.x] = s_pre[threadIdx.x];
    __syncthreads();
}
// prefixes -> order statistics -> what the select was for (one thread per column)
__device__ __forceinline__ void sel_finish_col(const SelArgs &a, FitScalars *sc, int c) {
    const double med = sel_median(sc, c);
    sc->sel_value[2 * c] = value_of(sc->sel_prefix[2 * c]);
    sc->sel_value[2 * c + 1] = value_of(sc->sel_prefix[2 * c + 1]);
    if (a.mode == SEL_RESID) {
        sc->med = med;
        sc->nres = sc->sel_count[c];
    } else if (a.mode == SEL_ABSDEV) {
        sc->mad = 1.4826 * med;  // R mad(): constant 1.4826
    } else {
        sc->sel_value[2 * c] = exp(med);  // size factor of column c
        if (a.sf_out) a.sf_out[c] = sc->sel_value[2 * c];
    }
}

// ---- sharded shortcut (protocol and layout: fit_state.h) -------------------------------------------------------
__global__ void sel_gcount_kernel(SelArgs a, FitWork w, int world, int rank) {
    const int nq = 2 * a.ncol;
    for (int k = threadIdx.x; k < world * nq; k += blockDim.x) {
        const int r = k / nq, q = k - r * nq;
        w.selcnt[k] = r == rank ? sel_local_count(w.sc, w.hist_local, q >> 1, q & 1) : 0.0;
    }
    if (threadIdx.x < (unsigned)nq) w.sc->sel_cnt[threadIdx.x] = 0;  // write positions of the place pass
    if (threadIdx.x == 0) w.sc->sel_fast_done = 0;
}
__device__ __forceinline__ bool sel_gather_fits(const double *cnt, int world, int nq) {
    for (int q = 0; q < nq; q++) {
        double t = 0;
        for (int r = 0; r < world; r++) t += cnt[(size_t)r * nq + q];
        if (t > (double)kSelCap) return false;
    }
    return true;
}
// this rank's candidates, as values, at its offset of the (zeroed) hist buffer; the sum-all-reduce then gathers
__global__ __launch_bounds__(256) void sel_gplace_kernel(SelArgs a, FitWork w, int world, int rank) {
    const int col = blockIdx.y, nq = 2 * a.ncol;
    FitScalars *sc = w.sc;
    if (!sel_gather_fits(w.selcnt, world, nq)) return;  // same verdict on every rank: the histogram rounds go on
    const uint64_t p0 = sc->sel_prefix[2 * col], p1 = sc->sel_prefix[2 * col + 1];
    const bool same = p0 == p1;
    double base[2], tot;
    sel_gather_layout(w.selcnt, world, rank, nq, 2 * col, &base[0], &tot);
    sel_gather_layout(w.selcnt, world, rank, nq, 2 * col + 1, &base[1], &tot);
    uint64_t key;
    for (int64_t i = blockIdx.x * 256 + threadIdx.x; i < a.n; i += (int64_t)gridDim.x * 256) {
        if (!sel_key(a, sc, col, i, key)) continue;
        int slot = -1;
        if (sel_match(key, p0, 40)) slot = 0;
        else if (!same && sel_match(key, p1, 40)) slot = 1;
        if (slot < 0) continue;
        const unsigned pos = atomicAdd(&sc->sel_cnt[2 * col + slot], 1u);
        w.hist[((size_t)2 * col + slot) * kSelCap + (size_t)base[slot] + pos] = value_of(key);
    }
}
__global__ __launch_bounds__(256) void sel_gfinish_kernel(SelArgs a, FitWork w, int world, int rank) {
    __shared__ uint64_t s_k[kSelCap];
    FitScalars *sc = w.sc;
    const int nq = 2 * a.ncol;
    if (!sel_gather_fits(w.selcnt, world, nq)) {
        if (blockIdx.x == 0 && threadIdx.x == 0) *(a.overflow_out ? a.overflow_out : &sc->sel_overflow) = 1;  // the host refits with every histogram round (api.hip)
        return;
    }
    const int col = blockIdx.x;
    const uint64_t p0 = sc->sel_prefix[2 * col], p1 = sc->sel_prefix[2 * col + 1];
    uint64_t result[2] = {p0, p1};
    for (int slot = 0; slot < 2; slot++) {
        const int hslot = (slot == 1 && p0 != p1) ? 1 : 0;
        double b, t;
        sel_gather_layout(w.selcnt, world, rank, nq, 2 * col + hslot, &b, &t);
        const int m = (int)t;
        if (m == 0) continue;
        int len = 64;
        while (len < m) len <<= 1;
        __syncthreads();
        for (int e = threadIdx.x; e < len; e += 256) s_k[e] = e < m ? key_of(w.hist[((size_t)2 * col + hslot) * kSelCap + e]) : ~0ull;
        __syncthreads();
        for (int k = 2; k <= len; k <<= 1)  // bitonic sort, ascending
            for (int j = k >> 1; j > 0; j >>= 1) {
                for (int e = threadIdx.x; e < len; e += 256) {
                    const int p = e ^ j;
                    if (p > e) {
                        const uint64_t x = s_k[e], y = s_k[p];
                        const bool up = (e & k) == 0;
                        if ((x > y) == up) { s_k[e] = y; s_k[p] = x; }
                    }
                }
                __syncthreads();
            }
        const int r = (int)sc->sel_rank[2 * col + slot];
        result[slot] = s_k[r < m ? r : m - 1];
        __syncthreads();
    }
    if (threadIdx.x == 0) {
        sc->sel_prefix[2 * col] = result[0];
        sc->sel_prefix[2 * col + 1] = result[1];
        if (col == 0) sc->sel_fast_done = 1;
    }
}

__global__ void sel_finish_kernel(SelArgs a, FitWork w) {
    if ((int)threadIdx.x < a.ncol) sel_finish_col(a, w.sc, threadIdx.x);
}

// workgroups per column: every workgroup ends with up to 2 x 4096 global atomics into the column's histogram, so
// more of them is not better — measured at 2 M rows: 512 for one column (MAD), 128 per column for eight (size factors)
static int sel_blocks(int64_t n, int ncol) {
    int64_t b = (n + 256 * 8 - 1) / (256 * 8);
    const int64_t cap = ncol >= 4 ? (1024 / ncol > 64 ? 1024 / ncol : 64) : 512;
    if (b < 1) b = 1;
    if (b > cap) b = cap;
    return (int)b;
}
void launch_sel_hist(SelArgs a, FitWork w, hipStream_t st) {
    const int bits = sel_bits(a.shift);
    (void)hipMemsetAsync(w.hist, 0, sizeof(double) * (size_t)a.ncol * 2 * kSelBins, st);
    sel_hist_kernel<<<dim3(sel_blocks(a.n, a.ncol), a.ncol), 256, 0, st>>>(a, w, bits);
}
void launch_sel_step(SelArgs a, FitWork w, hipStream_t st) {
    const int bits = sel_bits(a.shift);
    sel_step_kernel<<<a.ncol, 256, 0, st>>>(a, w, bits);
}
void launch_sel_shortcut(SelArgs a, FitWork w, hipStream_t st) {
    sel_compact_kernel<<<dim3(sel_blocks(a.n, a.ncol), a.ncol), 256, 0, st>>>(a, w);  // (sel_cnt was zeroed by the round-2 step)
    sel_small_kernel<<<a.ncol, 256, 0, st>>>(a, w);  // sort + pick, or the fallback rounds; then the column's finish
}
void launch_sel_finish(SelArgs a, FitWork w, hipStream_t st) { sel_finish_kernel<<<1, 64, 0, st>>>(a, w); }
void launch_sel_keep_local(SelArgs a, FitWork w, hipStream_t st) {
    (void)hipMemcpyAsync(w.hist_local, w.hist, sizeof(double) * (size_t)a.ncol * 2 * kSelBins, hipMemcpyDeviceToDevice, st);
}
void launch_sel_gather_counts(SelArgs a, FitWork w, int world, int rank, hipStream_t st) {
    sel_gcount_kernel<<<1, 256, 0, st>>>(a, w, world, rank);
}
void launch_sel_gather_place(SelArgs a, FitWork w, int world, int rank, hipStream_t st) {
    (void)hipMemsetAsync(w.hist, 0, sizeof(double) * (size_t)a.ncol * 2 * kSelCap, st);
    sel_gplace_kernel<<<dim3(sel_blocks(a.n, a.ncol), a.ncol), 256, 0, st>>>(a, w, world, rank);
}
void launch_sel_gather_finish(SelArgs a, FitWork w, int world, int rank, hipStream_t st) {
    sel_gfinish_kernel<<<a.ncol, 256, 0, st>>>(a, w, world, rank);
}

// ------------------------------------------------------------------------------------------

// a5 helper: the keys of the size-factor medians, computed once: ratio[j][i] = log(counts[j][i]) -
// rowMeans(log(counts))[i] for rows without a zero count (estimateSizeFactorsForMatrix uses only rows with
// a finite log geometric mean, and only positive counts), NaN otherwise.  The select passes then stream
// 8 B per element instead of recomputing a log.
__global__ __launch_bounds__(256) void row_ratio_kernel(const int32_t *__restrict__ counts, int64_t n, int S,
                                                        double *__restrict__ ratio, int32_t *clear_flag) {
    if (clear_flag && blockIdx.x == 0 && threadIdx.x == 0) *clear_flag = 0;
    for (int64_t i = blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256) {
        double s = 0;
        for (int j = 0; j < S; j++) {
            const double l = log((double)counts[(int64_t)j * n + i]);  // log(0) = -inf
            ratio[(int64_t)j * n + i] = l;
            s += l;
        }
        const double lg = s / S;
        const bool use = isfinite(lg);
        for (int j = 0; j < S; j++) ratio[(int64_t)j * n + i] = use ? ratio[(int64_t)j * n + i] - lg : NAN;
    }
}
__global__ __launch_bounds__(256) void row_ratio16_kernel(const int32_t *__restrict__ counts, int64_t n, int S,
                                                          double *__restrict__ ratio, int32_t *clear_flag) {
    if (clear_flag && blockIdx.x == 0 && threadIdx.x == 0) *clear_flag = 0;  // (the select that follows may set it)
    __shared__ LogEntry s_lt[64];
    log_table_to_lds(s_lt);
    const int64_t step = (int64_t)gridDim.x * 256;
    int32_t kn[16];  // the next row's counts are loaded before the current row is worked on
    int64_t i = blockIdx.x * 256 + threadIdx.x;
#pragma unroll
    for (int j = 0; j < 16; j++) kn[j] = (j < S && i < n) ? counts[(int64_t)j * n + i] : 1;
    for (; i < n; i += step) {
        double l[16];
        int32_t kc[16];
#pragma unroll
        for (int j = 0; j < 16; j++) kc[j] = kn[j];
        if (i + step < n) {
#pragma unroll
            for (int j = 0; j < 16; j++) kn[j] = j < S ? counts[(int64_t)j * n + i + step] : 1;
        }
#pragma unroll
        for (int j = 0; j < 16; j++) {
            const int32_t k = kc[j];
            l[j] = k > 0 ? tlog((double)k, s_lt) : (k == 0 ? -INFINITY : NAN);  // log(0) = -Inf drops the row, as in R
        }
        double s = 0;
#pragma unroll
        for (int j = 0; j < 16; j++)
            if (j < S) s += l[j];  // sample order, as the loop above
        const double lg = s / S;
        const bool use = isfinite(lg);
#pragma unroll
        for (int j = 0; j < 16; j++)
            if (j < S) ratio[(int64_t)j * n + i] = use ? l[j] - lg : NAN;
    }
}
void launch_row_ratio(const int32_t *counts, int64_t n, int S, double *ratio, int32_t *clear_flag, hipStream_t st) {
    if (S <= 16) row_ratio16_kernel<<<kRedBlocks * 2, 256, 0, st>>>(counts, n, S, ratio, clear_flag);
    else row_ratio_kernel<<<kRedBlocks, 256, 0, st>>>(counts, n, S, ratio, clear_flag);
}

// ---- size factors in two passes over the counts (single rank, S <= 16; common.h: sf_bin) -------------------------------------
// row_ratio16 + the radix select write the n x S keys once and read them three times (576 MB at 2 M x 8 for S medians).  A key is S
// table logarithms and a subtraction on a row that has to be read anyway, so here the counts are read twice and the keys recomputed:
//   sf_hist   every column's histogram of the keys' VALUE bins, in LDS, added to the global one
//   sf_pick   per column: population, the two middle ranks, the bin(s) that hold them and the ranks inside (and the global
//             histogram back to zero for the next call)
//   sf_list   the keys of the picked bins appended to the column's list (slot 0 from the front of its n words, slot 1 — the upper
//             middle's bin when it is another — from the back: together at most n keys, so a list cannot overflow whatever the ties)
//   sf_finish per column: the exact order statistics of the list(s), then sel_finish_col as the radix select ends
// Plain stream-ordered launches: no grid barrier, nothing that needs workgroups to be resident together.

// The keys of one row, by row_ratio16_kernel's expressions (-ffp-contract=off: the same bits wherever this is inlined — the two
// passes must agree on every key).  false = the row is not used (a zero or negative count).
// TAB (option "sf_log_table"): log k of a count 0 <= k < kSfLogK is read from logk[] — the table sf_logk_to_lds fills with this very
// expression, so the key has the same bits either way —, a larger or negative count goes through it under a branch (99.94 % of the
// benchmark matrix's counts are below 2048: a wave trip of 64 rows takes the branch for 4 % of its samples).  A count is an integer,
// and the row-per-thread passes are issue-bound: the ~25 VALU instructions of tlog per key were about half of both.
#ifndef CHICDIFF_SF_LOGK
#define CHICDIFF_SF_LOGK 2048
#endif
constexpr int kSfLogK = CHICDIFF_SF_LOGK;  // 16 KB of LDS; DESIGN.md section 5 has 1024 against 2048
__device__ __forceinline__ double sf_log_count(int32_t k, const LogEntry *lt) {
    return k > 0 ? tlog((double)k, lt) : (k == 0 ? -INFINITY : NAN);  // log(0) = -Inf drops the row, as in R
}
// (call behind log_table_to_lds; ends with a barrier)
__device__ __forceinline__ void sf_logk_to_lds(double *logk, const LogEntry *lt) {
    for (int k = threadIdx.x; k < kSfLogK; k += blockDim.x) logk[k] = sf_log_count(k, lt);
    __syncthreads();
}
template <int SM, bool TAB>
__device__ __forceinline__ bool sf_row_keys(const int32_t (&kc)[SM], int S, const LogEntry *lt, const double *logk, double (&x)[SM]) {
    double l[SM];
#pragma unroll
    for (int j = 0; j < SM; j++) {
        const int32_t k = kc[j];
        if (TAB && (uint32_t)k < (uint32_t)kSfLogK) l[j] = logk[k];
        else l[j] = sf_log_count(k, lt);
    }
    double s = 0;
#pragma unroll
    for (int j = 0; j < SM; j++)
        if (j < S) s += l[j];  // sample order
    const double lg = s / S;
#pragma unroll
    for (int j = 0; j < SM; j++) x[j] = l[j] - lg;
    return isfinite(lg);
}

// hist_add with an early way out: real data ties in a few values (a wave's lanes on one LDS word serialise), the benchmark's
// hardly at all — one look for a group of equal bins, more only while the groups found are worth it
__device__ __forceinline__ void sf_hist_add(unsigned int *h, bool valid, unsigned int bin) {
    unsigned long long todo = __ballot(valid);
    const int lane = threadIdx.x & 63;
    for (int it = 0; it < 4 && todo; it++) {
        const int leader = __ffsll((long long)todo) - 1;
        const unsigned int bl = (unsigned int)__builtin_amdgcn_readlane((int)bin, leader);  // (no LDS round trip: `leader` is wave-uniform)
        const unsigned long long same = __ballot(valid && bin == bl) & todo;
        const int cnt = __popcll(same);
        if (lane == leader) atomicAdd(&h[bl], (unsigned int)cnt);
        todo &= ~same;
        if (cnt < 4) break;
    }
    if ((todo >> lane) & 1ull) atomicAdd(&h[bin], 1u);
}

constexpr int kSfThreads = 1024;  // every launch of the route: workgroups of 16 waves
constexpr int kSfStage = 4096;    // keys a workgroup of sf_list stages in LDS before it reserves room in the lists
constexpr int kSfCntStride = 32;  // the lists' lengths (words behind the global histograms) lie 128 bytes apart

// The bin that holds 0-based rank r of a histogram of nb <= 4 x kSfThreads counters (LDS or global), for nr ranks at once: the first
// bin b with h[0] + ... + h[b] > r, else the last one (fit_state.h sel_pick; parallel as in mad_select: thread t owns `per`
// consecutive bins, a scan over the workgroup, the owning thread refines).  from_total: the ranks are the two middles of the
// histogram's own total.  Every thread of the workgroup calls it and gets the same answers; ends with a barrier.
__device__ __forceinline__ void sf_wg_pick(const unsigned int *h, int nb, int nr, bool from_total, double (&rank)[2], int (&bin)[2],
                                           double (&rin)[2], unsigned int (&cnt)[2], double &total_out) {
    __shared__ double sh_scan[kSfThreads / 64], sh_rin[2];
    __shared__ int sh_bin[2];
    __shared__ unsigned int sh_cnt[2];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int per = (nb + kSfThreads - 1) / kSfThreads;
    double mine[4] = {0, 0, 0, 0}, acc = 0;
#pragma unroll
    for (int q = 0; q < 4; q++) {
        const int b = tid * per + q;
        if (q < per && b < nb) mine[q] = (double)h[b];
        acc += mine[q];
    }
    double incl = acc;  // inclusive scan over the workgroup (counts: exact in fp64)
    for (int off = 1; off < 64; off <<= 1) {
        const double o = __shfl_up(incl, off);
        if (lane >= off) incl += o;
    }
    if (lane == 63) sh_scan[wave] = incl;
    __syncthreads();
    double before_wave = 0, total = 0;
    for (int q = 0; q < kSfThreads / 64; q++) {
        if (q < wave) before_wave += sh_scan[q];
        total += sh_scan[q];
    }
    incl += before_wave;
    const double before = incl - acc;
    const bool last_thread = tid == (nb - 1) / per;
    if (from_total) {  // R median(): the two middles
        const int64_t mi = (int64_t)total;
        rank[0] = (double)((mi - 1) / 2);
        rank[1] = (double)(mi / 2);
    }
    for (int s = 0; s < nr; s++) {
        const double r = rank[s];
        if ((before <= r && r < incl) || (last_thread && r >= incl && incl == total)) {
            double cum = before;
            int q = 0;
            for (; q < per - 1 && tid * per + q < nb - 1; q++) {
                if (cum + mine[q] > r) break;
                cum += mine[q];
            }
            sh_bin[s] = tid * per + q;
            sh_rin[s] = r - cum;
            sh_cnt[s] = (unsigned int)mine[q];
        }
    }
    __syncthreads();
    for (int s = 0; s < nr; s++) {
        bin[s] = sh_bin[s];
        rin[s] = sh_rin[s];
        cnt[s] = sh_cnt[s];
    }
    total_out = total;
    __syncthreads();  // (the shared words belong to the next call from here on)
}

template <int SM, bool TAB>
__global__ __launch_bounds__(kSfThreads) void sf_hist_kernel(const int32_t *__restrict__ counts, int64_t n, int S, int nb,
                                                            unsigned int *__restrict__ ghist, int32_t *clear_flag) {
    if (clear_flag && blockIdx.x == 0 && threadIdx.x == 0) *clear_flag = 0;  // (nothing on this route sets it: as row_ratio16_kernel)
    __shared__ LogEntry s_lt[64];
    __shared__ unsigned int s_h[kSfHistWords];
    __shared__ double s_logk[TAB ? kSfLogK : 1];
    const int words = S * nb;
    for (int k = threadIdx.x; k < words; k += kSfThreads) s_h[k] = 0;
    log_table_to_lds(s_lt);
    if (TAB) sf_logk_to_lds(s_logk, s_lt);
    const int64_t step = (int64_t)gridDim.x * kSfThreads;
    int32_t kn[SM];  // the next row's counts are loaded before the current row is worked on
    int64_t i = (int64_t)blockIdx.x * kSfThreads + threadIdx.x;
#pragma unroll
    for (int j = 0; j < SM; j++) kn[j] = (j < S && i < n) ? counts[(int64_t)j * n + i] : 1;
    for (; i < n; i += step) {
        int32_t kc[SM];
        double x[SM];
#pragma unroll
        for (int j = 0; j < SM; j++) kc[j] = kn[j];
        if (i + step < n) {
#pragma unroll
            for (int j = 0; j < SM; j++) kn[j] = j < S ? counts[(int64_t)j * n + i + step] : 1;
        }
        const bool use = sf_row_keys<SM, TAB>(kc, S, s_lt, s_logk, x);
#pragma unroll
        for (int j = 0; j < SM; j++)
            if (j < S) sf_hist_add(s_h + j * nb, use, (unsigned int)sf_bin(x[j], nb));
    }
    __syncthreads();
    for (int k = threadIdx.x; k < words; k += kSfThreads) {
        const unsigned int c = s_h[k];
        if (c) atomicAdd(&ghist[k], c);
    }
}

// what sf_pick leaves in the select's scalars for the two launches behind it: sel_count = population, sel_prefix[2 c + slot] = the
// bin of the slot's rank (nb, which no key has, for an empty population), sel_rank = the rank inside that bin; and the lengths of the
// column's two lists (gcnt) at zero
__global__ __launch_bounds__(kSfThreads) void sf_pick_kernel(FitWork w, unsigned int *ghist, unsigned int *gcnt, int nb) {
    const int col = blockIdx.x;
    FitScalars *sc = w.sc;
    unsigned int *g = ghist + (size_t)col * nb;
    double rank[2], rin[2], total;
    int bin[2];
    unsigned int cnt[2];
    sf_wg_pick(g, nb, 2, true, rank, bin, rin, cnt, total);
    for (int k = threadIdx.x; k < nb; k += kSfThreads) g[k] = 0;  // (every thread has read its bins: sf_wg_pick ends with a barrier)
    if (threadIdx.x < 2) {
        const int slot = threadIdx.x;
        sc->sel_prefix[2 * col + slot] = (uint64_t)(total > 0 ? bin[slot] : nb);
        sc->sel_rank[2 * col + slot] = rin[slot];
        gcnt[(2 * col + slot) * kSfCntStride] = 0;
        if (slot == 0) sc->sel_count[col] = total;
        if (slot == 0 && col == 0) sc->sel_fast_done = 0;
    }
}

// One atomic per wave and list straight into the lists' lengths made this launch 312 us at 2 M x 8: about every wave trip holds a
// wanted key, the returning atomics of 256 CUs queue on the one cache line the sixteen lengths shared.  So a workgroup keeps what it
// finds in LDS and reserves room once per list at its end; only keys beyond kSfStage (massive ties) go out at once, wave by wave.
template <int SM, bool TAB>
__global__ __launch_bounds__(kSfThreads) void sf_list_kernel(const int32_t *__restrict__ counts, int64_t n, int S, int nb, FitWork w,
                                                            unsigned int *__restrict__ gcnt, uint64_t *__restrict__ lists) {
    __shared__ LogEntry s_lt[64];
    __shared__ double s_logk[TAB ? kSfLogK : 1];
    __shared__ int s_b[2][kSfMaxS];
    __shared__ uint64_t s_key[kSfStage];
    __shared__ unsigned char s_tag[kSfStage];  // 2 x column + slot
    __shared__ unsigned int s_n, s_lc[2 * kSfMaxS], s_base[2 * kSfMaxS];
    const FitScalars *sc = w.sc;
    if ((int)threadIdx.x < 2 * S) s_b[threadIdx.x & 1][threadIdx.x >> 1] = (int)sc->sel_prefix[threadIdx.x];
    if (threadIdx.x < 2 * kSfMaxS) s_lc[threadIdx.x] = 0;
    if (threadIdx.x == 0) s_n = 0;
    log_table_to_lds(s_lt);
    if (TAB) sf_logk_to_lds(s_logk, s_lt);
    const int lane = threadIdx.x & 63;
    const int64_t step = (int64_t)gridDim.x * kSfThreads;
    int32_t kn[SM];
    int64_t i = (int64_t)blockIdx.x * kSfThreads + threadIdx.x;
#pragma unroll
    for (int j = 0; j < SM; j++) kn[j] = (j < S && i < n) ? counts[(int64_t)j * n + i] : 1;
    for (; i < n; i += step) {
        int32_t kc[SM];
        double x[SM];
#pragma unroll
        for (int j = 0; j < SM; j++) kc[j] = kn[j];
        if (i + step < n) {
#pragma unroll
            for (int j = 0; j < SM; j++) kn[j] = j < S ? counts[(int64_t)j * n + i + step] : 1;
        }
        const bool use = sf_row_keys<SM, TAB>(kc, S, s_lt, s_logk, x);
        unsigned int hit = 0;  // bit j: column j's key lies in the bin of slot 0; bit 16 + j: in that of slot 1, another bin
#pragma unroll
        for (int j = 0; j < SM; j++)
            if (j < S) {
                const int b = sf_bin(x[j], nb);
                const int b0 = s_b[0][j], b1 = s_b[1][j];
                hit |= (b == b0 ? 1u : 0u) << j;
                hit |= (b != b0 && b == b1 ? 1u : 0u) << (16 + j);
            }
        if (!use) hit = 0;
        unsigned int over = 0;  // the hits that found the stage full
        if (hit != 0) {
#pragma unroll
            for (int j = 0; j < SM; j++)
#pragma unroll
                for (int slot = 0; slot < 2; slot++)
                    if (j < S && ((hit >> (16 * slot + j)) & 1u)) {
                        const unsigned int pos = atomicAdd(&s_n, 1u);
                        if (pos < (unsigned int)kSfStage) {
                            s_key[pos] = key_of(x[j]);
                            s_tag[pos] = (unsigned char)(2 * j + slot);
                        } else over |= 1u << (16 * slot + j);
                    }
        }
        if (__ballot(over != 0) == 0ull) continue;
#pragma unroll
        for (int j = 0; j < SM; j++)
            if (j < S) {
#pragma unroll
                for (int slot = 0; slot < 2; slot++) {  // one atomic per wave and list: the leader reserves, every lane writes its own
                    const bool m = (over >> (16 * slot + j)) & 1u;
                    const unsigned long long mask = __ballot(m);
                    if (mask == 0ull) continue;
                    const int leader = __ffsll((long long)mask) - 1;
                    unsigned int base = 0;
                    if (lane == leader) base = atomicAdd(&gcnt[(2 * j + slot) * kSfCntStride], (unsigned int)__popcll(mask));
                    base = (unsigned int)__shfl((int)base, leader);
                    if (m) {
                        const int64_t pos = (int64_t)base + __popcll(mask & ((1ull << lane) - 1ull));
                        lists[(int64_t)j * n + (slot ? n - 1 - pos : pos)] = key_of(x[j]);
                    }
                }
            }
    }
    __syncthreads();
    const int staged = (int)(s_n < (unsigned int)kSfStage ? s_n : (unsigned int)kSfStage);
    for (int e = threadIdx.x; e < staged; e += kSfThreads) atomicAdd(&s_lc[s_tag[e]], 1u);
    __syncthreads();
    if ((int)threadIdx.x < 2 * S) {
        const unsigned int c = s_lc[threadIdx.x];
        s_base[threadIdx.x] = c ? atomicAdd(&gcnt[threadIdx.x * kSfCntStride], c) : 0u;
        s_lc[threadIdx.x] = 0;
    }
    __syncthreads();
    for (int e = threadIdx.x; e < staged; e += kSfThreads) {
        const int t = s_tag[e], j = t >> 1;
        const int64_t pos = (int64_t)s_base[t] + atomicAdd(&s_lc[t], 1u);
        lists[(int64_t)j * n + ((t & 1) ? n - 1 - pos : pos)] = s_key[e];
    }
}

constexpr int kSfCand = 1024;  // keys of one sub-bin that are ranked by counting; more (massive ties, keys beyond the binned range): radix rounds
__device__ __forceinline__ uint64_t sf_list_at(const uint64_t *list, int64_t n, bool back, int64_t e) { return list[back ? n - 1 - e : e]; }

// The keys of ranks rk[0 .. nr) (0-based, inside the list) of a list of m keys that all lie in value bin b.  One histogram of the
// keys' sub-bins (about one key each on the benchmark's data), the sub-bin of each rank picked, its few keys ranked by counting
// those in front of each (smaller, or equal with a lower index).  A sub-bin with more than kSfCand keys is massive ties or an end
// bin whose keys lie beyond the binned range: the rank is then found by the radix select's own six rounds over the key bits, the
// whole list scanned by this workgroup each round — slow and exact, as sel_tail_rounds is.  Results in s_res (LDS), behind a barrier.
__device__ __forceinline__ void sf_list_select(const uint64_t *list, int64_t n, bool back, int64_t m, int nb, int b, int nr,
                                               double (&rk)[2], unsigned int *s_h, uint64_t *s_c, unsigned int *s_nc, uint64_t *s_res) {
    const int tid = threadIdx.x;
    for (int k = tid; k < kSfSubBins; k += kSfThreads) s_h[k] = 0;
    __syncthreads();
    for (int64_t e = tid; e < m; e += kSfThreads)
        sf_hist_add(s_h, true, (unsigned int)sf_sub_bin(value_of(sf_list_at(list, n, back, e)), nb, b));
    __syncthreads();
    int sb[2];
    double rin[2], total;
    unsigned int cnt[2];
    sf_wg_pick(s_h, kSfSubBins, nr, false, rk, sb, rin, cnt, total);
    for (int q = 0; q < nr; q++) {
        const bool shared = nr == 2 && sb[0] == sb[1] && cnt[0] <= (unsigned int)kSfCand;  // both ranks off one set of candidates
        if (q == 1 && shared) break;
        if (cnt[q] <= (unsigned int)kSfCand) {
            if (tid == 0) *s_nc = 0;
            __syncthreads();
            for (int64_t e = tid; e < m; e += kSfThreads) {
                const uint64_t key = sf_list_at(list, n, back, e);
                if (sf_sub_bin(value_of(key), nb, b) == sb[q]) s_c[atomicAdd(s_nc, 1u)] = key;
            }
            __syncthreads();
            const int nc = (int)cnt[q];
            if (tid < nc) {
                const uint64_t mine = s_c[tid];
                int less = 0;
                for (int k = 0; k < nc; k++) {
                    const uint64_t o = s_c[k];
                    less += (o < mine || (o == mine && k < tid)) ? 1 : 0;
                }
                if ((double)less == rin[q]) s_res[q] = mine;
                if (shared && (double)less == rin[1]) s_res[1] = mine;
            }
            __syncthreads();
        } else {
            uint64_t p = 0;
            double r[2] = {rk[q], 0};
            for (int round = 0; round < 6; round++) {
                const int shift = kSelShifts[round], bits = sel_bits(shift), hi = shift + bits;
                const uint64_t dmask = (1ull << bits) - 1ull;
                for (int k = tid; k < kSelBins; k += kSfThreads) s_h[k] = 0;
                __syncthreads();
                for (int64_t e = tid; e < m; e += kSfThreads) {
                    const uint64_t key = sf_list_at(list, n, back, e);
                    sf_hist_add(s_h, sel_match(key, p, hi), (unsigned int)((key >> shift) & dmask));
                }
                __syncthreads();
                int rb[2];
                double rr[2], rt;
                unsigned int rc[2];
                sf_wg_pick(s_h, 1 << bits, 1, false, r, rb, rr, rc, rt);
                p |= (uint64_t)rb[0] << shift;
                r[0] = rr[0];
            }
            if (tid == 0) s_res[q] = p;
            __syncthreads();
        }
    }
}

__global__ __launch_bounds__(kSfThreads) void sf_finish_kernel(SelArgs a, FitWork w, int nb, const unsigned int *__restrict__ gcnt,
                                                              const uint64_t *__restrict__ lists) {
    __shared__ unsigned int s_h[kSelBins > kSfSubBins ? kSelBins : kSfSubBins];
    __shared__ uint64_t s_c[kSfCand], s_res[2];
    __shared__ unsigned int s_nc;
    const int col = blockIdx.x;
    FitScalars *sc = w.sc;
    const int b0 = (int)sc->sel_prefix[2 * col], b1 = (int)sc->sel_prefix[2 * col + 1];
    const double rank0 = sc->sel_rank[2 * col], rank1 = sc->sel_rank[2 * col + 1];
    const int64_t m0 = gcnt[2 * col * kSfCntStride], m1 = gcnt[(2 * col + 1) * kSfCntStride];
    const bool empty = !(sc->sel_count[col] > 0);
    const uint64_t *list = lists + (int64_t)col * a.n;
    // (an empty population ends on the prefixes the radix select's rounds leave for one: a NaN pattern; the median is NaN by sel_count)
    if (threadIdx.x < 2) s_res[threadIdx.x] = 0xFFFFFF0000000000ull;
    __syncthreads();
    if (!empty) {
        if (b0 == b1) {
            double rk[2] = {rank0, rank1};
            const int nr = rank0 == rank1 ? 1 : 2;
            sf_list_select(list, a.n, false, m0, nb, b0, nr, rk, s_h, s_c, &s_nc, s_res);
            if (nr == 1 && threadIdx.x == 0) s_res[1] = s_res[0];
        } else {  // the two middles of an even population in different bins: a list each
            double rk[2] = {rank0, 0};
            sf_list_select(list, a.n, false, m0, nb, b0, 1, rk, s_h, s_c, &s_nc, s_res);
            rk[0] = rank1;
            sf_list_select(list, a.n, true, m1, nb, b1, 1, rk, s_h, s_c, &s_nc, s_res + 1);
        }
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        sc->sel_prefix[2 * col] = s_res[0];
        sc->sel_prefix[2 * col + 1] = s_res[1];
        if (col == 0) sc->sel_fast_done = 1;
        sel_finish_col(a, sc, col);  // size factor of the column, as the radix select ends
    }
}

template <bool TAB>
static void launch_sf_passes(const int32_t *counts, int64_t n, int S, int nb, unsigned int hb, FitWork w, unsigned int *hist, unsigned int *gcnt,
                             uint64_t *lists, int32_t *clear_flag, hipStream_t st) {
    if (S <= 4) sf_hist_kernel<4, TAB><<<hb, kSfThreads, 0, st>>>(counts, n, S, nb, hist, clear_flag);
    else if (S <= 8) sf_hist_kernel<8, TAB><<<hb, kSfThreads, 0, st>>>(counts, n, S, nb, hist, clear_flag);
    else sf_hist_kernel<16, TAB><<<hb, kSfThreads, 0, st>>>(counts, n, S, nb, hist, clear_flag);
    sf_pick_kernel<<<S, kSfThreads, 0, st>>>(w, hist, gcnt, nb);
    if (S <= 4) sf_list_kernel<4, TAB><<<hb, kSfThreads, 0, st>>>(counts, n, S, nb, w, gcnt, lists);
    else if (S <= 8) sf_list_kernel<8, TAB><<<hb, kSfThreads, 0, st>>>(counts, n, S, nb, w, gcnt, lists);
    else sf_list_kernel<16, TAB><<<hb, kSfThreads, 0, st>>>(counts, n, S, nb, w, gcnt, lists);
}
void launch_sf_direct(const int32_t *counts, int64_t n, int S, SelArgs a, FitWork w, unsigned int *hist, uint64_t *lists,
                      int32_t *clear_flag, int cus, int log_table, hipStream_t st) {
    const int nb = sf_bins(S);
    // both passes: one 16-wave workgroup per CU and a grid-stride loop.  LDS (62 KB, 78 with the table of log k) would let a second one in, registers do not (65 at
    // S = 8: a SIMD holds seven such waves, two workgroups need eight); and every workgroup of pass 1 ends by adding its S x nb
    // counters to the global histogram, so more of them is more of that
    int64_t hb = (n + kSfThreads - 1) / kSfThreads;
    if (hb > (cus > 0 ? cus : 256)) hb = cus > 0 ? cus : 256;
    unsigned int *gcnt = hist + kSfHistWords;
    if (log_table) launch_sf_passes<true>(counts, n, S, nb, (unsigned)hb, w, hist, gcnt, lists, clear_flag, st);
    else launch_sf_passes<false>(counts, n, S, nb, (unsigned)hb, w, hist, gcnt, lists, clear_flag, st);
    sf_finish_kernel<<<S, kSfThreads, 0, st>>>(a, w, nb, gcnt, lists);
}

}  // namespace cd
