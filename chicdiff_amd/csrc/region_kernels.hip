// region_kernels.hip — the HBM-bound Chicdiff-side kernels of the region stages.
//
//  * offsets (chicdiff.R:1583-1589, 1635-1638), window sums (:1540-1547), count join (:843-858);
//  * per-fragment background (:628-703 + Chicago .estimateBMean/.distFun);
//  * region assembly: count join, background and window sums of a region in one kernel, without
//    the fragment matrices.
#include "common.h"
#include "devmath.h"
#include "prior_mc.h"

namespace cd {

// a4: offsets.  One thread per row.  For S <= 16 the row lives in registers (one HBM read, one write);
// larger S re-reads the row from L1/L2.  log() keeps R's semantics for NA/0/negative inputs, the
// common positive-finite case takes the cheaper flog().
__device__ __forceinline__ double rlog(double x) { return (x > 0.0 && x < 1.7e308) ? flog(x) : log(x); }

// 2 S logarithms, 2 exponentials and 2 S quotients per row sit beside 16 S bytes of traffic: the kernel is only
// HBM-bound if that arithmetic is lean — table-driven log (devmath.h tlog, 1 KB table in LDS) and one reciprocal per
// geometric mean instead of S divisions.  Measured against 50-digit values (tests/test_gpu_norm.py, profiles/r29_norm_accuracy.json),
// in the units of tests/norm_twin.py (unmixed: 2^-53 (1 + mean_j |log x_j|), relative): worst 2.98 unmixed and 0.71 mixed over
// S = 2 .. 16, where the library log and a division per element (the oracle; offsets_kernel below for S > 16) reach 2.82 and 0.65
// on the same elements.
// N: the sample class (S <= N, 4 / 8 / 16, picked at launch as sf_hist_kernel's) — the row's register array is as long as the class, not
// always 16 doubles (compile-time resource report of the build: DESIGN.md section 5, round 18)
template <int N>
__global__ __launch_bounds__(256) void offsets16_kernel(const double *__restrict__ fm, const double *__restrict__ sf,
                                                        int64_t n, int S, double theta, int mix,
                                                        double *__restrict__ out) {
    __shared__ LogEntry s_lt[64];
    log_table_to_lds(s_lt);
    for (int64_t i = blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256) {
        double v[N];
#pragma unroll
        for (int j = 0; j < N; j++) v[j] = j < S ? fm[(int64_t)j * n + i] : 1.0;
        offsets_row16<N>(v, S, sf, theta, mix, s_lt);
#pragma unroll
        for (int j = 0; j < N; j++)
            if (j < S) out[(int64_t)j * n + i] = v[j];
    }
}

__global__ __launch_bounds__(256) void offsets_kernel(const double *__restrict__ fm, const double *__restrict__ sf,
                                                      int64_t n, int S, double theta, int mix,
                                                      double *__restrict__ out) {
    for (int64_t i = blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256) {
        double sl = 0;
        for (int j = 0; j < S; j++) sl += rlog(fm[(int64_t)j * n + i]);
        const double gmean = exp(sl / S);
        bool anyna = false;
        for (int j = 0; j < S; j++) {
            const double m3 = fm[(int64_t)j * n + i] / gmean;
            anyna |= (m3 != m3);
        }
        double g2 = 1.0;
        if (mix) {
            double sl2 = 0;
            for (int j = 0; j < S; j++) {
                const double m3 = anyna ? sf[j] : fm[(int64_t)j * n + i] / gmean;
                sl2 += rlog(m3 * (1 - theta) + sf[j] * theta);
            }
            g2 = exp(sl2 / S);
        }
        for (int j = 0; j < S; j++) {
            double m3 = anyna ? sf[j] : fm[(int64_t)j * n + i] / gmean;
            if (mix) m3 = (m3 * (1 - theta) + sf[j] * theta) / g2;
            out[(int64_t)j * n + i] = m3;
        }
    }
}
// norm = "standard" (chicdiff.R:1572-1575): the size factors themselves, one column per sample
__global__ __launch_bounds__(256) void offsets_sf_kernel(const double *__restrict__ sf, int64_t n, int S, double *__restrict__ out) {
    for (int64_t i = blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256)
        for (int j = 0; j < S; j++) out[(int64_t)j * n + i] = sf[j];
}
void launch_offsets(const double *fm, const double *sf_dev, int64_t n, int S, double theta, int mix, double *out,
                    hipStream_t st) {
    int64_t blocks = (n + 255) / 256;
    if (blocks > 4096) blocks = 4096;
    if (!fm) {
        offsets_sf_kernel<<<(unsigned)blocks, 256, 0, st>>>(sf_dev, n, S, out);
        return;
    }
    if (S <= 4)
        offsets16_kernel<4><<<(unsigned)blocks, 256, 0, st>>>(fm, sf_dev, n, S, theta, mix, out);
    else if (S <= 8)
        offsets16_kernel<8><<<(unsigned)blocks, 256, 0, st>>>(fm, sf_dev, n, S, theta, mix, out);
    else if (S <= 16)
        offsets16_kernel<16><<<(unsigned)blocks, 256, 0, st>>>(fm, sf_dev, n, S, theta, mix, out);
    else
        offsets_kernel<<<(unsigned)blocks, 256, 0, st>>>(fm, sf_dev, n, S, theta, mix, out);
}

// a2: window sums.  A block owns 256 consecutive regions of one sample; their fragments are one
// contiguous range (regions are contiguous fragment windows), which the block streams into LDS
// with coalesced loads; each thread then adds up its own window from LDS, in fragment order
// (sequential fp64 sum = the order sum() sees after setkey(otherEndID)).  Windows whose span does
// not fit the staging buffer (never for RUexpand <= 5) take the direct path.
constexpr int kWinCap = 256 * 12;  // staged fragments per block (F <= 11 for the default RUexpand = 5)
__global__ __launch_bounds__(256) void window_sums_kernel(const int32_t *__restrict__ fragN,
                                                          const double *__restrict__ fragFM, int64_t nfrag, int S,
                                                          const int64_t *__restrict__ rptr, int64_t n,
                                                          int32_t *__restrict__ N, double *__restrict__ FM) {
    __shared__ int32_t s_n[kWinCap];
    __shared__ double s_f[kWinCap];
    const int j = blockIdx.y;
    const int64_t nblk = (n + 255) / 256;
    for (int64_t blk = blockIdx.x; blk < nblk; blk += gridDim.x) {
        const int64_t i0 = blk * 256, i1 = (i0 + 256 < n) ? i0 + 256 : n;
        const int64_t f0 = rptr[i0], f1 = rptr[i1];
        const int64_t i = i0 + threadIdx.x;
        const bool staged = (f1 - f0) <= kWinCap;
        int64_t lo = 0, hi = 0;
        if (i < i1) { lo = rptr[i]; hi = rptr[i + 1]; }
        if (staged) {
            __syncthreads();  // previous iteration's readers are done with the buffers
            // all 12 loads of a thread are issued before the first LDS store (memory-level parallelism)
            const int span = (int)(f1 - f0);
            if (fragN) {
                int32_t v[12];
#pragma unroll
                for (int k = 0; k < 12; k++) {
                    const int e = threadIdx.x + k * 256;
                    v[k] = e < span ? fragN[(int64_t)j * nfrag + f0 + e] : 0;
                }
#pragma unroll
                for (int k = 0; k < 12; k++) {
                    const int e = threadIdx.x + k * 256;
                    if (e < span) s_n[e] = v[k];
                }
            }
            if (fragFM) {
                double v[12];
#pragma unroll
                for (int k = 0; k < 12; k++) {
                    const int e = threadIdx.x + k * 256;
                    v[k] = e < span ? fragFM[(int64_t)j * nfrag + f0 + e] : 0.0;
                }
#pragma unroll
                for (int k = 0; k < 12; k++) {
                    const int e = threadIdx.x + k * 256;
                    if (e < span) s_f[e] = v[k];
                }
            }
            __syncthreads();
            if (i < i1) {
                if (fragN) {
                    int32_t s = 0;
                    for (int64_t f = lo; f < hi; f++) s += s_n[f - f0];
                    N[(int64_t)j * n + i] = s;
                }
                if (fragFM) {
                    double s = 0;
                    for (int64_t f = lo; f < hi; f++) s += s_f[f - f0];
                    FM[(int64_t)j * n + i] = s;
                }
            }
        } else if (i < i1) {
            if (fragN) {
                int32_t s = 0;
                for (int64_t f = lo; f < hi; f++) s += fragN[(int64_t)j * nfrag + f];
                N[(int64_t)j * n + i] = s;
            }
            if (fragFM) {
                double s = 0;
                for (int64_t f = lo; f < hi; f++) s += fragFM[(int64_t)j * nfrag + f];
                FM[(int64_t)j * n + i] = s;
            }
        }
    }
}
void launch_window_sums(const int32_t *fragN, const double *fragFM, int64_t nfrag, int S, const int64_t *rptr,
                        int64_t n, int32_t *N, double *FM, hipStream_t st) {
    int64_t blocks = (n + 255) / 256;
    if (blocks > 1024) blocks = 1024;  // x S samples in grid.y: >> 256 CUs
    window_sums_kernel<<<dim3((unsigned)blocks, S), 256, 0, st>>>(fragN, fragFM, nfrag, S, rptr, n, N, FM);
}

// a1: count join.  RU is keyed by baitID (chicdiff.R:425) and a region's fragments are consecutive IDs, so the 512
// queries of a wave's tile (eight consecutive rows per lane, moved as 4 x int32) fall in a narrow key range.  Each
// wave works alone — no block barrier — and keeps the chain of DEPENDENT global loads per tile short, which is what
// bounds the kernel (measured at 22 M queries x 10 M keys: a block-wide LDS window 0.31 ms, one global binary search
// per query 0.24 ms, a per-lane register run of 16 keys 0.17 ms):
//   1. lo = lower bound of the tile's smallest query: a 64-ary search by the whole wave over the table's coarse
//      level (every 64th key, copied out once per call: 1/64 of the table, L2-resident), then one dense load of
//      the 64 keys it points at — probing the table itself every 64th key costs a 128-byte line per 8 bytes used
//      and two to three HBM round trips per tile;
//   2. one dense load of the next 64 coarse entries bounds the tile's largest query: hi
//      (a tile that spans more than 4096 keys gets a proper search instead);
//   3. a range of at most kJoinCap keys goes to the wave's LDS slice with its values (coalesced, read once) and
//      every lane resolves its eight queries there by a branch-free binary search, eight independent LDS reads per
//      step; a wider range (a far denser table, an unsorted caller) is searched in global memory the same way;
//   4. key and value at the lower bound decide match / no match (N <- 0, chicdiff.R:851-853).
// Results do not depend on the tiling or on the path taken.
// kJoinCap = 768 (round 5; 512 before): a table nearly as dense as RU (the end-to-end leg: 19 M keys under 21.5 M rows) sent every
// other tile through the global search — 0.20 ms at 22 M x 19.8 M against 0.135 with the wider window, four blocks per CU instead of
// six; a sparser table (10 M keys) is unchanged at 0.117.  Tried on the way and dropped (no gain: the tile's chain of dependent loads
// is NOT what bounds the kernel any more): runs of consecutive tiles per wave with the last tile's answer as a hint for the next.
constexpr int kJoinPerLane = 8, kJoinTile = 64 * kJoinPerLane, kJoinCap = 768;
// lower_bound over keys[lo, hi) by the 64 lanes of a wave; every lane returns the same value
__device__ __forceinline__ int64_t wave_lower_bound(const int64_t *__restrict__ keys, int64_t lo, int64_t hi, int64_t target, int lane) {
    while (hi - lo > 64) {
        const int64_t step = (hi - lo + 63) / 64;
        const int64_t pos = lo + (int64_t)lane * step;
        const int c = __popcll(__ballot(pos < hi && keys[pos] < target));  // monotone in the lane
        const int64_t nlo = c > 0 ? lo + (int64_t)(c - 1) * step + 1 : lo;
        const int64_t pc = lo + (int64_t)c * step;
        hi = pc < hi ? pc : hi;  // the answer is in [nlo, hi] (it may be `hi` itself)
        lo = nlo;
    }
    const int64_t pos = lo + lane;
    return lo + __popcll(__ballot(pos < hi && keys[pos] < target));
}

// One tile's 512 queries (eight per lane, q[]; kmin / kmax = the tile's smallest / largest, wave-uniform) against ONE sorted key table:
// steps 1-4 above.  sk / sv = the wave's LDS slice.  Shared by the single-table and the all-replicates kernels.
__device__ __forceinline__ void join_tile_table(const int64_t (&q)[kJoinPerLane], int64_t kmin, int64_t kmax, const int64_t *__restrict__ keys,
                                                const int32_t *__restrict__ vals, int64_t nkeys, const int64_t *__restrict__ index, int64_t nidx,
                                                int64_t *sk, int32_t *sv, int lane, int32_t (&res)[kJoinPerLane]) {
    // lo: the coarse level (every 64th key, L2-resident) says which 64 keys hold the lower bound of the tile's
    // smallest query, one dense load of those finishes; hi: the first coarse entry >= the largest query, from the
    // 64 entries after lo (one dense load), or a proper search for a tile that spans more than 4096 keys
    const int64_t jlo = wave_lower_bound(index, 0, nidx, kmin, lane);  // first j with keys[64 j] >= kmin
    int64_t lo = 0;
    if (jlo > 0) {
        const int64_t e = 64 * jlo < nkeys ? 64 * jlo : nkeys;
        lo = wave_lower_bound(keys, 64 * (jlo - 1) + 1, e, kmin, lane);
    }
    int64_t hi;
    {
        const int64_t j0 = lo / 64 + 1, pos = j0 + lane;
        const int c = __popcll(__ballot(pos < nidx && index[pos] < kmax));
        int64_t jhi = j0 + c;  // keys[64 jhi] >= kmax, or jhi >= nidx
        if (c == 64) jhi = wave_lower_bound(index, j0 + 64, nidx, kmax, lane);
        hi = jhi < nidx ? 64 * jhi + 1 : nkeys;
    }
    if (hi - lo <= kJoinCap) {
        const int w = (int)(hi - lo);
        {
            int64_t tk[kJoinCap / 64];
            int32_t tv[kJoinCap / 64];
#pragma unroll
            for (int e = 0; e < kJoinCap / 64; e++) {
                const int at = e * 64 + lane;
                tk[e] = at < w ? keys[lo + at] : 0;
                tv[e] = at < w ? vals[lo + at] : 0;
            }
#pragma unroll
            for (int e = 0; e < kJoinCap / 64; e++) {
                sk[e * 64 + lane] = tk[e];
                sv[e * 64 + lane] = tv[e];
            }
        }
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
        __builtin_amdgcn_wave_barrier();
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
        int b[kJoinPerLane];  // the answer of query k stays in [b[k], b[k] + len]
#pragma unroll
        for (int k = 0; k < kJoinPerLane; k++) b[k] = 0;
        int len = w;
        while (len > 1) {
            const int half = len >> 1;
#pragma unroll
            for (int k = 0; k < kJoinPerLane; k++) b[k] += sk[b[k] + half - 1] < q[k] ? half : 0;
            len -= half;
        }
        if (len == 1) {
#pragma unroll
            for (int k = 0; k < kJoinPerLane; k++) b[k] += sk[b[k]] < q[k] ? 1 : 0;
        }
#pragma unroll
        for (int k = 0; k < kJoinPerLane; k++) {
            const bool in = b[k] < w;
            const int at = in ? b[k] : 0;
            res[k] = (in && sk[at] == q[k]) ? sv[at] : 0;
        }
        __builtin_amdgcn_wave_barrier();  // the slice is rewritten by the next tile
    } else {
        int64_t b[kJoinPerLane];
#pragma unroll
        for (int k = 0; k < kJoinPerLane; k++) b[k] = lo;
        int64_t len = hi - lo;
        while (len > 1) {
            const int64_t half = len >> 1;
#pragma unroll
            for (int k = 0; k < kJoinPerLane; k++) b[k] += keys[b[k] + half - 1] < q[k] ? half : 0;
            len -= half;
        }
#pragma unroll
        for (int k = 0; k < kJoinPerLane; k++) b[k] += keys[b[k]] < q[k] ? 1 : 0;  // len == 1: the range has > kJoinCap keys
#pragma unroll
        for (int k = 0; k < kJoinPerLane; k++) {
            const bool in = b[k] < hi;
            const int64_t at = in ? b[k] : lo;
            res[k] = (in && keys[at] == q[k]) ? vals[at] : 0;
        }
    }
}
// a tile's queries: eight consecutive RU rows per lane -> q[], and the tile's smallest / largest key (wave-uniform)
template <bool VEC>
__device__ __forceinline__ void join_tile_queries(const int32_t *__restrict__ bait, const int32_t *__restrict__ oe, int64_t nru, int64_t r0,
                                                  int64_t (&q)[kJoinPerLane], int64_t &kmin, int64_t &kmax) {
    int32_t qb[kJoinPerLane], qo[kJoinPerLane];
    if (VEC) {
        const int4 b0 = *(const int4 *)(bait + r0), b1 = *(const int4 *)(bait + r0 + 4);
        const int4 o0 = *(const int4 *)(oe + r0), o1 = *(const int4 *)(oe + r0 + 4);
        qb[0] = b0.x; qb[1] = b0.y; qb[2] = b0.z; qb[3] = b0.w; qb[4] = b1.x; qb[5] = b1.y; qb[6] = b1.z; qb[7] = b1.w;
        qo[0] = o0.x; qo[1] = o0.y; qo[2] = o0.z; qo[3] = o0.w; qo[4] = o1.x; qo[5] = o1.y; qo[6] = o1.z; qo[7] = o1.w;
    } else {
#pragma unroll
        for (int k = 0; k < kJoinPerLane; k++) {
            const bool v = r0 + k < nru;
            qb[k] = v ? bait[r0 + k] : 0;
            qo[k] = v ? oe[r0 + k] : 0;
        }
    }
    kmin = INT64_MAX;
    kmax = INT64_MIN;
#pragma unroll
    for (int k = 0; k < kJoinPerLane; k++) {
        q[k] = ((int64_t)qb[k] << 32) | (uint32_t)qo[k];
        if (VEC || r0 + k < nru) {
            kmin = q[k] < kmin ? q[k] : kmin;
            kmax = q[k] > kmax ? q[k] : kmax;
        }
    }
    for (int off = 32; off > 0; off >>= 1) {
        const int64_t a = __shfl_xor(kmin, off), c = __shfl_xor(kmax, off);
        kmin = a < kmin ? a : kmin;
        kmax = c > kmax ? c : kmax;
    }
}
template <bool VEC>
__device__ __forceinline__ void join_tile_store(int32_t *__restrict__ out, int64_t nru, int64_t r0, const int32_t (&res)[kJoinPerLane]) {
    if (VEC) {
        *(int4 *)(out + r0) = make_int4(res[0], res[1], res[2], res[3]);
        *(int4 *)(out + r0 + 4) = make_int4(res[4], res[5], res[6], res[7]);
    } else {
#pragma unroll
        for (int k = 0; k < kJoinPerLane; k++)
            if (r0 + k < nru) out[r0 + k] = res[k];
    }
}

// A full tile's 512 results to a column that is only 4-byte aligned (column t of an S x nru matrix starts at t * nru: 16-byte aligned
// for one nru in four).  The tile is one contiguous run of 2 KB; with k = the number of leading elements up to the next 16-byte
// boundary (wave-uniform: r0 is a multiple of 8), lane L stores the ALIGNED eight elements [8 L + k, 8 L + k + 8) — its own res[k..7]
// and the next lane's res[0..k-1] — as 2 x int4; lane 0 adds the tile's first k elements, lane 63 keeps its last 8 - k, as dwords.
__device__ __forceinline__ void join_tile_store_shifted(int32_t *__restrict__ col, int64_t r0, int lane, const int32_t (&res)[kJoinPerLane]) {
    const int k = (int)((4u - (unsigned)(((uintptr_t)(col + r0)) >> 2)) & 3u);  // same in every lane
    if (k == 0) {
        *(int4 *)(col + r0) = make_int4(res[0], res[1], res[2], res[3]);
        *(int4 *)(col + r0 + 4) = make_int4(res[4], res[5], res[6], res[7]);
        return;
    }
    const int n0 = __shfl_down(res[0], 1), n1 = __shfl_down(res[1], 1), n2 = __shfl_down(res[2], 1);
    int32_t v[kJoinPerLane];
    if (k == 1) { v[0] = res[1]; v[1] = res[2]; v[2] = res[3]; v[3] = res[4]; v[4] = res[5]; v[5] = res[6]; v[6] = res[7]; v[7] = n0; }
    else if (k == 2) { v[0] = res[2]; v[1] = res[3]; v[2] = res[4]; v[3] = res[5]; v[4] = res[6]; v[5] = res[7]; v[6] = n0; v[7] = n1; }
    else { v[0] = res[3]; v[1] = res[4]; v[2] = res[5]; v[3] = res[6]; v[4] = res[7]; v[5] = n0; v[6] = n1; v[7] = n2; }
    int32_t *dst = col + r0 + k;
    if (lane < 63) {
        *(int4 *)dst = make_int4(v[0], v[1], v[2], v[3]);
        *(int4 *)(dst + 4) = make_int4(v[4], v[5], v[6], v[7]);
    } else {
        for (int i = 0; i < kJoinPerLane - k; i++) dst[i] = v[i];
    }
    if (lane == 0)
        for (int i = 0; i < k; i++) col[r0 + i] = res[i];
}

// (gfx950: 160 KB of LDS per CU — the four waves' slices take 4 x 768 x 12 = 36 864 bytes per workgroup, so FOUR workgroups = 16 waves
// are resident per CU, which is what the launch bound asks the register allocator for; with the 512-key window it was six)
template <bool VEC>  // VEC: bait / oe / out are 16-byte aligned, full tiles move as 4 x int32
__global__ __launch_bounds__(256, 4) void count_join_kernel(const int32_t *__restrict__ bait, const int32_t *__restrict__ oe,
                                                         int64_t nru, const int64_t *__restrict__ keys,
                                                         const int32_t *__restrict__ vals, int64_t nkeys,
                                                         const int64_t *__restrict__ index, int64_t nidx,
                                                         int32_t *__restrict__ out) {
    __shared__ int64_t s_keys[4][kJoinCap];
    __shared__ int32_t s_vals[4][kJoinCap];
    const int lane = threadIdx.x & 63;
    int64_t *const sk = s_keys[threadIdx.x >> 6];
    int32_t *const sv = s_vals[threadIdx.x >> 6];
    // VEC launches cover the full tiles only; the ragged end (and unaligned callers) go through the scalar variant
    const int64_t ntile = VEC ? nru / kJoinTile : (nru + kJoinTile - 1) / kJoinTile;
    // blocks b and b + 8 share an XCD (round-robin dispatch; speed only): each of the eight L2s serves one contiguous
    // eighth of the tiles, so the sparse probes of neighbouring tiles (every 64th key: 128-byte lines of which 8
    // bytes are used) hit lines a neighbour has just brought in instead of going to HBM again
    const int64_t per_xcd = (ntile + 7) / 8, t_begin = (int64_t)(blockIdx.x & 7) * per_xcd;
    const int64_t t_end = t_begin + per_xcd < ntile ? t_begin + per_xcd : ntile;
    const int64_t wave0 = (int64_t)(blockIdx.x >> 3) * 4 + (threadIdx.x >> 6), nwave = (int64_t)(gridDim.x >> 3) * 4;
    for (int64_t tile = t_begin + wave0; tile < t_end; tile += nwave) {
        const int64_t r0 = tile * kJoinTile + (int64_t)lane * kJoinPerLane;
        int64_t q[kJoinPerLane], kmin, kmax;
        join_tile_queries<VEC>(bait, oe, nru, r0, q, kmin, kmax);
        int32_t res[kJoinPerLane];
        join_tile_table(q, kmin, kmax, keys, vals, nkeys, index, nidx, sk, sv, lane, res);
        join_tile_store<VEC>(out, nru, r0, res);
    }
}

// a1 for ALL replicates in one pass (round 6): chicdiff.R:843-858 is a loop over the replicates, each merge() reading the same RU
// rows; here a tile's (baitID, otherEndID) pairs are read ONCE and resolved against every replicate's key table in turn — per set of
// S joins 8 nru + S (4 nru + 12 nkeys) bytes instead of S (12 nru + 12 nkeys) (S = 8, 21.5 M rows, 19 M keys: 2.7 instead of 3.9 GB),
// one launch instead of S, and the coarse levels of all tables built by one launch.  Same per-table steps (join_tile_table): same bits.
constexpr int kJoinMaxTables = 16;  // per launch (the tables' pointers travel as kernel arguments); more replicates: several launches
struct JoinTables {
    const int64_t *keys[kJoinMaxTables];
    const int32_t *vals[kJoinMaxTables];
    const int64_t *index[kJoinMaxTables];
    int64_t nkeys[kJoinMaxTables];
    int32_t T;
};
template <bool VEC>
__global__ __launch_bounds__(256, 4) void count_join_multi_kernel(const int32_t *__restrict__ bait, const int32_t *__restrict__ oe, int64_t nru,
                                                                  JoinTables tb, int32_t *__restrict__ out, int64_t out_stride) {
    __shared__ int64_t s_keys[4][kJoinCap];
    __shared__ int32_t s_vals[4][kJoinCap];
    const int lane = threadIdx.x & 63;
    int64_t *const sk = s_keys[threadIdx.x >> 6];
    int32_t *const sv = s_vals[threadIdx.x >> 6];
    const int64_t ntile = VEC ? nru / kJoinTile : (nru + kJoinTile - 1) / kJoinTile;
    const int64_t per_xcd = (ntile + 7) / 8, t_begin = (int64_t)(blockIdx.x & 7) * per_xcd;
    const int64_t t_end = t_begin + per_xcd < ntile ? t_begin + per_xcd : ntile;
    const int64_t wave0 = (int64_t)(blockIdx.x >> 3) * 4 + (threadIdx.x >> 6), nwave = (int64_t)(gridDim.x >> 3) * 4;
    for (int64_t tile = t_begin + wave0; tile < t_end; tile += nwave) {
        const int64_t r0 = tile * kJoinTile + (int64_t)lane * kJoinPerLane;
        int64_t q[kJoinPerLane], kmin, kmax;
        join_tile_queries<VEC>(bait, oe, nru, r0, q, kmin, kmax);
#pragma unroll 1
        for (int t = 0; t < tb.T; t++) {
            int32_t res[kJoinPerLane];
            const int64_t nk = tb.nkeys[t];
            join_tile_table(q, kmin, kmax, tb.keys[t], tb.vals[t], nk, tb.index[t], (nk + 63) / 64, sk, sv, lane, res);
            int32_t *col = out + (int64_t)t * out_stride;
            if (VEC) join_tile_store_shifted(col, r0, lane, res);
            else join_tile_store<false>(col, nru, r0, res);
        }
    }
}
__global__ __launch_bounds__(256) void join_index_kernel(const int64_t *__restrict__ keys, int64_t nidx, int64_t *__restrict__ index) {
    const int64_t j = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (j < nidx) index[j] = keys[64 * j];
}
size_t count_join_scratch_bytes(int64_t nkeys) { return sizeof(int64_t) * (size_t)((nkeys + 63) / 64 + 1); }
// scratch: count_join_scratch_bytes(nkeys) bytes
void launch_count_join(const int32_t *bait, const int32_t *oe, int64_t nru, const int64_t *keys, const int32_t *vals,
                       int64_t nkeys, int32_t *out, void *scratch, hipStream_t st) {
    auto grid = [](int64_t rows) {  // a multiple of 8: one share of the tiles per XCD
        int64_t blocks = (((rows + kJoinTile - 1) / kJoinTile + 3) / 4 + 7) / 8 * 8;
        return (unsigned)(blocks > 8192 ? 8192 : (blocks < 8 ? 8 : blocks));
    };
    int64_t *index = (int64_t *)scratch;
    const int64_t nidx = (nkeys + 63) / 64;
    if (nidx > 0) join_index_kernel<<<(unsigned)((nidx + 255) / 256), 256, 0, st>>>(keys, nidx, index);
    const bool vec = (((uintptr_t)bait | (uintptr_t)oe | (uintptr_t)out) & 15) == 0;
    const int64_t body = vec ? nru / kJoinTile * kJoinTile : 0;
    if (body > 0) count_join_kernel<true><<<grid(body), 256, 0, st>>>(bait, oe, body, keys, vals, nkeys, index, nidx, out);
    if (nru > body)
        count_join_kernel<false><<<grid(nru - body), 256, 0, st>>>(bait + body, oe + body, nru - body, keys, vals, nkeys, index, nidx, out + body);
}

// all tables' coarse levels in one launch: grid.y = table
__global__ __launch_bounds__(256) void join_index_multi_kernel(JoinTables tb) {
    const int t = blockIdx.y;
    const int64_t nidx = (tb.nkeys[t] + 63) / 64;
    int64_t *index = const_cast<int64_t *>(tb.index[t]);
    for (int64_t j = (int64_t)blockIdx.x * 256 + threadIdx.x; j < nidx; j += (int64_t)gridDim.x * 256) index[j] = tb.keys[t][64 * j];
}
size_t count_join_multi_scratch_bytes(int S, const int64_t *nkeys) {
    size_t b = 0;
    for (int s = 0; s < S; s++) b += count_join_scratch_bytes(nkeys[s]);
    return b;
}
// out: S x nru (replicate-major); keys / vals / nkeys: host arrays of S entries (device pointers inside); scratch: count_join_multi_scratch_bytes
void launch_count_join_multi(const int32_t *bait, const int32_t *oe, int64_t nru, int S, const int64_t *const *keys, const int32_t *const *vals,
                             const int64_t *nkeys, int32_t *out, void *scratch, hipStream_t st) {
    auto grid = [](int64_t rows) {
        int64_t blocks = (((rows + kJoinTile - 1) / kJoinTile + 3) / 4 + 7) / 8 * 8;
        return (unsigned)(blocks > 8192 ? 8192 : (blocks < 8 ? 8 : blocks));
    };
    int64_t *index = (int64_t *)scratch;
    for (int s0 = 0; s0 < S; s0 += kJoinMaxTables) {
        JoinTables tb{};
        tb.T = S - s0 < kJoinMaxTables ? S - s0 : kJoinMaxTables;
        int64_t maxidx = 0;
        for (int t = 0; t < tb.T; t++) {
            tb.keys[t] = keys[s0 + t];
            tb.vals[t] = vals[s0 + t];
            tb.nkeys[t] = nkeys[s0 + t];
            tb.index[t] = index;
            const int64_t nidx = (nkeys[s0 + t] + 63) / 64;
            index += nidx + 1;
            maxidx = nidx > maxidx ? nidx : maxidx;
        }
        if (maxidx > 0) {
            int64_t bx = (maxidx + 255) / 256;
            join_index_multi_kernel<<<dim3((unsigned)(bx > 1024 ? 1024 : bx), tb.T), 256, 0, st>>>(tb);
        }
        int32_t *o = out + (int64_t)s0 * nru;
        const bool vec = (((uintptr_t)bait | (uintptr_t)oe) & 15) == 0;  // (the columns of `out` need not be: join_tile_store_shifted)
        const int64_t body = vec ? nru / kJoinTile * kJoinTile : 0;
        if (body > 0) count_join_multi_kernel<true><<<grid(body), 256, 0, st>>>(bait, oe, body, tb, o, nru);
        if (nru > body) count_join_multi_kernel<false><<<grid(nru - body), 256, 0, st>>>(bait + body, oe + body, nru - body, tb, o + body, nru);
    }
}

// a3: per-fragment background (chicdiff.R:628-703 + Chicago .estimateBMean/.distFun): a gather from
// dense per-fragment tables plus one log and one exp per (RU row, replicate).  HBM/L2-gather bound.
struct BgArgs {
    const int32_t *bait, *oe;
    int64_t nru;
    int32_t id_min, nid, S, ntblb, ntlb;
    const int64_t *midsum;
    const double *sj, *si;
    const int32_t *tblb, *tlb;
    const double *T;
    const double *distfun;  // device, S x 10
    double *bmean, *tmean, *fullmean;
};
// What bounds it (round 5, 22 M rows x 8 replicates, FullMean only: 0.95 ms = 1.7 TB/s of algorithmic bytes; profiles/r05_fragment_background_ablation.txt):
// instruction issue, not memory — 830 vector + 420 scalar instructions per 64 rows (SQ_INSTS_VALU / SQ_INSTS_SALU), HBM traffic 0.53 GB
// read + 1.375 GB written (as computed: every XCD reads the tables once).  Without the gathers 0.76 ms, without the stores 0.74, without
// either and without the midpoints 0.58.  Measured and NOT taken, each within +-2 % of the kernel below: the gathers of four replicates
// issued together, table-driven exp / log (devmath.h) in place of the device library's, the Tmean tables in LDS.
// One thread per RU row, the replicates in a loop (round 5; before: one thread per (row, replicate), grid.y = S): the row's two
// fragment IDs, the two midpoints and log|distance| are the same for every replicate — S - 1 of every S logarithms, ID loads and
// midpoint gathers were repeats — and a caller that wants FullMean alone (chicdiff.R:896: the one column DESeq2Wrap reads) passes
// NULL for the other two and saves two thirds of the stores.  Same expressions in the same order: same bits.
// The body of a3, shared by fragment_background_kernel and region_assemble_kernel (the library is built with -ffp-contract=off: the
// same expressions in the same order give the same bits wherever they are inlined).
// bg_row_geometry: what is the same for every replicate — the two fragments' indices into the dense tables, whether both are on
// the map, and log|distance| (0 where they are not: never read).
__device__ __forceinline__ bool bg_row_geometry(const BgArgs &a, int32_t bait, int32_t oe, int32_t &b, int32_t &o, double &ld) {
    // (32-bit subtractions: with id_min >= 1 and nid < 2^31 - id_min a difference that wraps round is >= 2^31 - id_min > nid, so it
    // cannot land inside [0, nid); the region universe's window is another matter, see ru_window.h)
    b = bait - a.id_min;
    o = oe - a.id_min;
    const bool on_map = b >= 0 && b < a.nid && o >= 0 && o < a.nid;
    ld = 0.0;
    if (on_map) {
        const double dist = rint((double)(a.midsum[o] - a.midsum[b]) / 2.0);  // R round(): half to even
        ld = log(fabs(dist));
    }
    return on_map;
}
// bg_row_replicate: Bmean and Tmean of one row for replicate s; p = the replicate's ten distance-function parameters
__device__ __forceinline__ void bg_row_replicate(const BgArgs &a, const double *p, int s, int32_t b, int32_t o, bool on_map, double ld,
                                                 double &B, double &Tm) {
    B = NAN;
    Tm = NAN;
    if (on_map) {
        const double s_j = a.sj[(int64_t)s * a.nid + b];
        double s_i = a.si[(int64_t)s * a.nid + o];
        if (s_i != s_i) s_i = 1.0;
        double e;
        if (ld > p[9]) e = p[6] + ld * p[7];
        else if (ld < p[8]) e = p[4] + ld * p[5];
        else e = p[0] + p[1] * ld + p[2] * (ld * ld) + p[3] * (ld * ld * ld);
        B = s_j * s_i * exp(e);
        const int32_t tb = a.tblb[(int64_t)s * a.nid + b], tl = a.tlb[(int64_t)s * a.nid + o];
        if (tb >= 0 && tl >= 0) {
            Tm = a.T[((int64_t)s * a.ntblb + tb) * a.ntlb + tl];
        } else if (tb >= 0) {
            double m = INFINITY;
            for (int k = 0; k < a.ntlb; k++) {
                const double v = a.T[((int64_t)s * a.ntblb + tb) * a.ntlb + k];
                if (v == v && v < m) m = v;
            }
            Tm = isfinite(m) ? m : NAN;
        }
    }
}
__global__ __launch_bounds__(256) void fragment_background_kernel(BgArgs a) {
    extern __shared__ double s_df[];  // S x 10: the replicates' distance functions
    for (int k = threadIdx.x; k < 10 * a.S; k += 256) s_df[k] = a.distfun[k];
    __syncthreads();
    for (int64_t r = blockIdx.x * 256 + threadIdx.x; r < a.nru; r += (int64_t)gridDim.x * 256) {
        int32_t b, o;
        double ld;
        const bool on_map = bg_row_geometry(a, a.bait[r], a.oe[r], b, o, ld);
        for (int s = 0; s < a.S; s++) {
            double B, Tm;
            bg_row_replicate(a, s_df + 10 * s, s, b, o, on_map, ld, B, Tm);
            if (a.bmean) a.bmean[(int64_t)s * a.nru + r] = B;
            if (a.tmean) a.tmean[(int64_t)s * a.nru + r] = Tm;
            if (a.fullmean) a.fullmean[(int64_t)s * a.nru + r] = B + Tm;
        }
    }
}
void launch_fragment_background(const int32_t *bait, const int32_t *oe, int64_t nru, int32_t id_min, int32_t nid,
                                const int64_t *midsum, int32_t S, const double *sj, const double *si, const int32_t *tblb,
                                const int32_t *tlb, const double *T, int32_t ntblb, int32_t ntlb, const double *distfun_dev,
                                double *bmean, double *tmean, double *fullmean, hipStream_t st) {
    BgArgs a{bait, oe, nru, id_min, nid, S, ntblb, ntlb, midsum, sj, si, tblb, tlb, T, distfun_dev, bmean, tmean, fullmean};
    int64_t blocks = (nru + 255) / 256;
    if (blocks > 8192) blocks = 8192;
    if (blocks < 1) blocks = 1;
    fragment_background_kernel<<<(unsigned)blocks, 256, sizeof(double) * 10 * S, st>>>(a);
}

// a1 + a3 + a2 in one kernel (chinput branch only: chicdiff.R:843-858, 628-703, 894-896, 1540-1547): region-level N and FullMean
// straight from the RU rows, the replicates' key tables and the Chicago background tables.  Neither per-fragment matrix exists:
// per region 8 F bytes read for the RU rows (F = fragments per region) + 12 nkeys / n per replicate for the tables, 12 S written,
// against 8 F + 12 S F written and 12 S F read again by count_join_multi -> fragment_background -> window_sums.
// Equal to those three calls bit for bit: the join is join_tile_table (its result does not depend on which lane holds which
// query), FullMean is bg_row_geometry / bg_row_replicate, and a lane adds up its region's rows one after the other in ascending
// row order from 0 / 0.0, as window_sums_kernel does.  The branch without chinput files (count_join_inner: Reduce(merge) semantics,
// a pair counts only where every replicate holds it) comes here through the merged tables of launch_count_merge below.
// Work unit: a wave owns a tile of kAsmRegions consecutive regions = the consecutive RU rows rptr[i0] .. rptr[i1].
//   * kAsmRegions = 46: with the default RUexpand = 5 a region has at most 11 rows, so 46 regions (506 rows) fill the 512-row
//     join tile; the tiling is fixed (region i belongs to tile i / 46), so no scan and no host read decides it.
//   * tile path (the tile's rows fit the join tile): row f0 + 64 k + lane goes to query k of the lane (coalesced dword loads — region
//     starts are not 16-byte aligned), log|distance| is formed once per row; then per replicate FullMean of the rows, and after
//     that per replicate the join: either to the wave's LDS slice, where lane k < 46 adds up region i0 + k and stores.  The value
//     buffer (512 x 12 bytes) overlays the key window (768 x 12 bytes), which is dead once join_tile_table has returned, and
//     log|distance| waits in the window's other half while FullMean is formed: 36 864 bytes per workgroup + the distance
//     functions, four workgroups = 16 waves per CU as count_join_multi_kernel (107 registers, no scratch).
//   * generic path (a tile with more rows — a caller's own CSR with long regions — or the test option region_assemble_generic):
//     lane k walks region i0 + k row by row, one binary search over the whole table per row and replicate.  The choice is
//     wave-uniform and made here from rptr.
// Row indices come from the caller's rptr: rows outside [0, nru) are never read (they count as absent).
constexpr int kAsmRegions = 46;
__device__ __forceinline__ int64_t uniform64(int64_t x) {  // a wave-uniform value, moved to scalar registers
    const uint32_t l = __builtin_amdgcn_readfirstlane((uint32_t)x), h = __builtin_amdgcn_readfirstlane((uint32_t)((uint64_t)x >> 32));
    return (int64_t)(((uint64_t)h << 32) | l);
}
struct RegionAssembleArgs {
    const int32_t *bait, *oe;
    int64_t nru;
    const int64_t *rptr;
    int64_t n;
    JoinTables tb;  // the tables of this launch: replicates s0 .. s0 + tb.T - 1
    BgArgs bg;      // the background tables of ALL replicates (bait / oe / nru / outputs unused); distfun = S x 10 on the device
    int32_t s0, force_generic;
    int32_t *N;  // n x S column-major, either may be NULL
    double *FM;
};
__global__ __launch_bounds__(256, 4) void region_assemble_kernel(RegionAssembleArgs a) {
    __shared__ __align__(16) char s_slice[4][kJoinCap * 12];
    __shared__ double s_df[kJoinMaxTables * 10];
    static_assert(2 * kJoinTile * 8 <= kJoinCap * 12 && kJoinTile * 4 <= kJoinCap * 4, "the value buffers overlay the key window");
    const int T = a.tb.T;
    if (a.FM)
        for (int k = threadIdx.x; k < 10 * T; k += 256) s_df[k] = a.bg.distfun[10 * a.s0 + k];
    __syncthreads();
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);  // scalar: so are the tile, its regions and its row range below
    char *const slice = s_slice[wave];
    int64_t *const sk = reinterpret_cast<int64_t *>(slice);  // key window: keys, then values
    int32_t *const sv = reinterpret_cast<int32_t *>(slice + kJoinCap * 8);
    double *const vf = reinterpret_cast<double *>(slice);    // value buffer, over it: FullMean where the keys were, N where the values were
    int32_t *const vn = sv;
    double *const vl = vf + kJoinTile;                       // ... and, until the joins start, the rows' log|distance| after FullMean
    const int64_t ntile = (a.n + kAsmRegions - 1) / kAsmRegions;
    // one contiguous share of the tiles per XCD, as count_join_kernel (blocks b and b + 8 share an XCD)
    const int64_t per_xcd = (ntile + 7) / 8, t_begin = (int64_t)(blockIdx.x & 7) * per_xcd;
    const int64_t t_end = t_begin + per_xcd < ntile ? t_begin + per_xcd : ntile;
    // ONE tile per wave, no loop over tiles: around such a loop the compiler keeps the loop-invariant lane addresses and the
    // constants of log / exp in registers across the joins — 128 registers and spills to scratch; without it 107 and none
    const int64_t tile = t_begin + (int64_t)(blockIdx.x >> 3) * 4 + wave;
    if (tile < t_end) {
        const int lane = threadIdx.x & 63;
        const int64_t i0 = tile * kAsmRegions;
        const int nreg = a.n - i0 < kAsmRegions ? (int)(a.n - i0) : kAsmRegions;
        int64_t lo = 0, hi = 0;
        if (lane < nreg) {
            lo = a.rptr[i0 + lane];
            hi = a.rptr[i0 + lane + 1];
        }
        const int64_t f0 = a.rptr[i0], f1 = a.rptr[i0 + nreg];  // (wave-uniform: scalar loads)
        const int64_t rows = f1 - f0;
        if (!a.force_generic && rows >= 0 && rows <= kJoinTile) {
            int64_t q[kJoinPerLane], kmin = INT64_MAX, kmax = INT64_MIN;
            unsigned on_map = 0;
#pragma unroll
            for (int k = 0; k < kJoinPerLane; k++) {
                const int64_t r = f0 + k * 64 + lane;
                const bool v = k * 64 + lane < rows && r >= 0 && r < a.nru;
                const int32_t qb = v ? a.bait[r] : 0, qo = v ? a.oe[r] : 0;
                q[k] = ((int64_t)qb << 32) | (uint32_t)qo;
                if (v) {
                    kmin = q[k] < kmin ? q[k] : kmin;
                    kmax = q[k] > kmax ? q[k] : kmax;
                }
                if (a.FM) {  // log|distance| waits in the lane's own words of the slice (the key window is idle until the joins)
                    int32_t b, o;
                    double ld = 0.0;
                    if (v && bg_row_geometry(a.bg, qb, qo, b, o, ld)) on_map |= 1u << k;
                    vl[k * 64 + lane] = ld;
                }
            }
            for (int off = 32; off > 0; off >>= 1) {
                const int64_t x = __shfl_xor(kmin, off), y = __shfl_xor(kmax, off);
                kmin = x < kmin ? x : kmin;
                kmax = y > kmax ? y : kmax;
            }
            kmin = uniform64(kmin);  // (the same in every lane: scalar registers from here on)
            kmax = uniform64(kmax);
            // the lane's region as a range of the value buffer
            int64_t l64 = lo < f0 ? f0 : lo, h64 = hi > f1 ? f1 : hi;
            const int l_ = (int)(l64 - f0), lh = l_ | ((h64 < l64 ? l_ : (int)(h64 - f0)) << 16);  // both <= 512: one register
            // the replicates twice, FullMean first and then the joins: the joins' key windows need the whole slice and most of the
            // 128 registers that 16 waves per CU leave a lane
            if (a.FM) {
#pragma unroll 1
                for (int t = 0; t < T; t++) {
#pragma unroll
                    for (int k = 0; k < kJoinPerLane; k++) {
                        double B, Tm;
                        bg_row_replicate(a.bg, s_df + 10 * t, a.s0 + t, (int32_t)(q[k] >> 32) - a.bg.id_min, (int32_t)q[k] - a.bg.id_min,
                                         (on_map >> k) & 1u, vl[k * 64 + lane], B, Tm);
                        vf[k * 64 + lane] = B + Tm;
                    }
                    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
                    __builtin_amdgcn_wave_barrier();
                    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
                    if (lane < nreg) {
                        double s = 0;
                        for (int f = lh & 0xffff, h = lh >> 16; f < h; f++) s += vf[f];
                        a.FM[(int64_t)(a.s0 + t) * a.n + i0 + lane] = s;
                    }
                    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
                    __builtin_amdgcn_wave_barrier();  // the buffer is rewritten by the next replicate
                }
            }
            if (a.N) {
#pragma unroll 1
                for (int t = 0; t < T; t++) {
                    int32_t res[kJoinPerLane];
                    if (kmin <= kmax) {  // (wave-uniform; a tile of empty regions asks nothing)
                        const int64_t nk = a.tb.nkeys[t];
                        join_tile_table(q, kmin, kmax, a.tb.keys[t], a.tb.vals[t], nk, a.tb.index[t], (nk + 63) / 64, sk, sv, lane, res);
                    } else {
#pragma unroll
                        for (int k = 0; k < kJoinPerLane; k++) res[k] = 0;
                    }
#pragma unroll
                    for (int k = 0; k < kJoinPerLane; k++) vn[k * 64 + lane] = res[k];
                    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
                    __builtin_amdgcn_wave_barrier();
                    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
                    if (lane < nreg) {
                        int32_t s = 0;
                        for (int f = lh & 0xffff, h = lh >> 16; f < h; f++) s += vn[f];
                        a.N[(int64_t)(a.s0 + t) * a.n + i0 + lane] = s;
                    }
                    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
                    __builtin_amdgcn_wave_barrier();  // the slice is rewritten by the next replicate's key window
                }
            }
        } else if (lane < nreg) {
            const int64_t l = lo < 0 ? 0 : lo, h = hi > a.nru ? a.nru : hi;
#pragma unroll 1
            for (int t = 0; t < T; t++) {
                const int64_t col = (int64_t)(a.s0 + t) * a.n + i0 + lane;
                const int64_t *const keys = a.tb.keys[t];
                const int64_t nk = a.tb.nkeys[t];
                int32_t sN = 0;
                double sF = 0;
                for (int64_t r = l; r < h; r++) {
                    const int32_t qb = a.bait[r], qo = a.oe[r];
                    if (a.N) {
                        const int64_t key = ((int64_t)qb << 32) | (uint32_t)qo;
                        int64_t at = 0, len = nk;
                        while (len > 0) {
                            const int64_t half = len >> 1;
                            if (keys[at + half] < key) {
                                at += half + 1;
                                len -= half + 1;
                            } else {
                                len = half;
                            }
                        }
                        sN += (at < nk && keys[at] == key) ? a.tb.vals[t][at] : 0;
                    }
                    if (a.FM) {
                        int32_t b, o;
                        double ldr, B, Tm;
                        const bool on = bg_row_geometry(a.bg, qb, qo, b, o, ldr);
                        bg_row_replicate(a.bg, s_df + 10 * t, a.s0 + t, b, o, on, ldr, B, Tm);
                        sF += B + Tm;
                    }
                }
                if (a.N) a.N[col] = sN;
                if (a.FM) a.FM[col] = sF;
            }
        }
    }
}
// keys / vals / nkeys: host arrays of S entries (device pointers inside), NULL when N is; the background tables when FM is not NULL;
// scratch: count_join_multi_scratch_bytes.  Returns the first launch error (hipGetLastError right after each launch).
hipError_t launch_region_assemble(const int32_t *bait, const int32_t *oe, int64_t nru, const int64_t *rptr, int64_t n, int S,
                                  const int64_t *const *keys, const int32_t *const *vals, const int64_t *nkeys, int32_t id_min, int32_t nid,
                                  const int64_t *midsum, const double *sj, const double *si, const int32_t *tblb, const int32_t *tlb,
                                  const double *T, int32_t ntblb, int32_t ntlb, const double *distfun_dev, int32_t *N, double *FM,
                                  void *scratch, int force_generic, hipStream_t st) {
    const int64_t ntile = (n + kAsmRegions - 1) / kAsmRegions;
    const int64_t blocks = 8 * (((ntile + 7) / 8 + 3) / 4);  // a wave per tile; blocks b, b + 8, ... serve one XCD's contiguous share
    int64_t *index = (int64_t *)scratch;
    for (int s0 = 0; s0 < S; s0 += kJoinMaxTables) {
        RegionAssembleArgs a{};
        a.bait = bait;
        a.oe = oe;
        a.nru = nru;
        a.rptr = rptr;
        a.n = n;
        a.tb.T = S - s0 < kJoinMaxTables ? S - s0 : kJoinMaxTables;
        a.bg = BgArgs{nullptr, nullptr, 0, id_min, nid, S, ntblb, ntlb, midsum, sj, si, tblb, tlb, T, distfun_dev, nullptr, nullptr, nullptr};
        a.s0 = s0;
        a.force_generic = force_generic;
        a.N = N;
        a.FM = FM;
        if (N) {
            int64_t maxidx = 0;
            for (int t = 0; t < a.tb.T; t++) {
                a.tb.keys[t] = keys[s0 + t];
                a.tb.vals[t] = vals[s0 + t];
                a.tb.nkeys[t] = nkeys[s0 + t];
                a.tb.index[t] = index;
                const int64_t nidx = (nkeys[s0 + t] + 63) / 64;
                index += nidx + 1;
                maxidx = nidx > maxidx ? nidx : maxidx;
            }
            if (maxidx > 0) {
                const int64_t bx = (maxidx + 255) / 256;
                join_index_multi_kernel<<<dim3((unsigned)(bx > 1024 ? 1024 : bx), a.tb.T), 256, 0, st>>>(a.tb);
                if (hipError_t e = hipGetLastError()) return e;
            }
        }
        region_assemble_kernel<<<(unsigned)blocks, 256, 0, st>>>(a);
        if (hipError_t e = hipGetLastError()) return e;
    }
    return hipSuccess;
}

// a1 without chinput files, the merge itself (chicdiff.R:778, the Reduce(merge) of :774-807 and :1202-1260): mergedFiles = the pairs
// that EVERY replicate's table holds, each with its S counts, formed once per call of getFullRegionData.  The left join of the chinput
// branch (count_join_multi, region_assemble) against the merged tables then IS the inner join of this branch, bit for bit: a pair absent
// from any replicate is absent from the merged table and gets 0 in every replicate, a pair held by all keeps each replicate's N.
//   * pivot = the table with the fewest keys (the first of them on a tie; the host knows nkeys).  Only its keys can be in the result,
//     and the result is the intersection, so it does not depend on which table that is.
//   * mark pass (count_merge_mark_kernel): a wave owns a tile of kJoinTile consecutive pivot keys, eight per lane as the RU rows of the
//     count join, and tests them against every other table in turn.  Tile and table are sorted, so the tile maps to one narrow key
//     range per table: the coarse level, wave_lower_bound, the key window in the wave's LDS slice and the branch-free searches are
//     join_tile_table's (join_tile_hits below, its sibling without values).  A hit is KEY EQUALITY at the lower bound — a table may hold
//     N = 0, which join_tile_table's result cannot tell from "absent".  The hits are ANDed over the tables; once no query of the tile
//     is alive the wave leaves the tile (wave-uniform), so disjoint tables cost one table's test.  Out: one flag byte per lane (bit k =
//     pivot key 8 lane + k is kept; 64 bytes = 512 flag bits per tile) and the tile's count.  More than kJoinMaxTables other tables:
//     several launches, the flag bytes carry the mask from one batch to the next.
//   * one rocPRIM exclusive scan of the tile counts (launch_scan_i64, in place): every tile's first output row, and behind the last
//     tile n_out — the one value the host waits for.
//   * write pass (count_merge_write_kernel): output row = the tile's first row + the key's rank among the tile's kept keys (one ballot
//     and popcount per flag bit).  The key and the pivot's value come from the pivot's own columns; every other table's value comes from
//     resolving the tile again with join_tile_table itself — for a kept key the value at its lower bound.  Tiles that keep nothing
//     are skipped.  Why not positions stored by the mark pass: per pivot key and table they cost 8 bytes written and 8 read again plus a
//     4-byte gather that touches the same lines of the value column, against 8 bytes of the key window read again (L2 / Infinity
//     Cache warm from the mark pass) + 4 of values read coalesced; the traffic is about equal, the (S - 1) x npivot x 8 bytes of
//     scratch are not needed, and the write pass runs the very function whose result the downstream joins must reproduce.
// Placement is by the scan alone: no value and no position passes through an atomic, so the output does not depend on the launch
// shape or on the order in which waves arrive.  Rows are 64-bit throughout.
__device__ __forceinline__ uint32_t join_tile_hits(const int64_t (&q)[kJoinPerLane], int64_t kmin, int64_t kmax, const int64_t *__restrict__ keys,
                                                   int64_t nkeys, const int64_t *__restrict__ index, int64_t nidx, int64_t *sk, int lane) {
    // [lo, hi): join_tile_table's steps 1 and 2
    const int64_t jlo = wave_lower_bound(index, 0, nidx, kmin, lane);
    int64_t lo = 0;
    if (jlo > 0) {
        const int64_t e = 64 * jlo < nkeys ? 64 * jlo : nkeys;
        lo = wave_lower_bound(keys, 64 * (jlo - 1) + 1, e, kmin, lane);
    }
    int64_t hi;
    {
        const int64_t j0 = lo / 64 + 1, pos = j0 + lane;
        const int c = __popcll(__ballot(pos < nidx && index[pos] < kmax));
        int64_t jhi = j0 + c;
        if (c == 64) jhi = wave_lower_bound(index, j0 + 64, nidx, kmax, lane);
        hi = jhi < nidx ? 64 * jhi + 1 : nkeys;
    }
    uint32_t hits = 0;
    if (hi - lo <= kJoinCap) {
        const int w = (int)(hi - lo);
        {
            int64_t tk[kJoinCap / 64];
#pragma unroll
            for (int e = 0; e < kJoinCap / 64; e++) {
                const int at = e * 64 + lane;
                tk[e] = at < w ? keys[lo + at] : 0;
            }
#pragma unroll
            for (int e = 0; e < kJoinCap / 64; e++) sk[e * 64 + lane] = tk[e];
        }
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
        __builtin_amdgcn_wave_barrier();
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
        int b[kJoinPerLane];
#pragma unroll
        for (int k = 0; k < kJoinPerLane; k++) b[k] = 0;
        int len = w;
        while (len > 1) {
            const int half = len >> 1;
#pragma unroll
            for (int k = 0; k < kJoinPerLane; k++) b[k] += sk[b[k] + half - 1] < q[k] ? half : 0;
            len -= half;
        }
        if (len == 1) {
#pragma unroll
            for (int k = 0; k < kJoinPerLane; k++) b[k] += sk[b[k]] < q[k] ? 1 : 0;
        }
#pragma unroll
        for (int k = 0; k < kJoinPerLane; k++) {
            const bool in = b[k] < w;
            const int at = in ? b[k] : 0;
            hits |= (in && sk[at] == q[k]) ? 1u << k : 0u;
        }
        __builtin_amdgcn_wave_barrier();  // the slice is rewritten by the next table
    } else {
        int64_t b[kJoinPerLane];
#pragma unroll
        for (int k = 0; k < kJoinPerLane; k++) b[k] = lo;
        int64_t len = hi - lo;
        while (len > 1) {
            const int64_t half = len >> 1;
#pragma unroll
            for (int k = 0; k < kJoinPerLane; k++) b[k] += keys[b[k] + half - 1] < q[k] ? half : 0;
            len -= half;
        }
#pragma unroll
        for (int k = 0; k < kJoinPerLane; k++) b[k] += keys[b[k]] < q[k] ? 1 : 0;  // len == 1: the range has > kJoinCap keys
#pragma unroll
        for (int k = 0; k < kJoinPerLane; k++) {
            const bool in = b[k] < hi;
            const int64_t at = in ? b[k] : lo;
            hits |= (in && keys[at] == q[k]) ? 1u << k : 0u;
        }
    }
    return hits;
}
struct CountMergeArgs {
    const int64_t *pkeys;  // the pivot: np keys, np >= 1
    const int32_t *pvals;
    int64_t np;
    JoinTables tb;                  // the other tables of this launch
    int32_t col[kJoinMaxTables];    // ... and the output column of each
    int32_t pcol, first, vec;       // the pivot's column; first launch of its pass; pkeys is 16-byte aligned
    uint8_t *flags;                 // ntile x 64
    int64_t *start;                 // ntile + 1: the tiles' counts (mark), scanned in place to their first rows (write)
    int64_t cap;
    int64_t *keys_out;
    int32_t *vals_out;
};
// a tile's pivot keys -> q[] (the rows behind the table's end repeat its last key: any value inside the tile's key range will do,
// their flag bits are never set), which of them exist, and the tile's smallest / largest key: its first and last (the table is sorted)
__device__ __forceinline__ uint32_t merge_tile_keys(const CountMergeArgs &a, int64_t tile, int lane, int64_t (&q)[kJoinPerLane], int64_t &kmin,
                                                    int64_t &kmax) {
    const int64_t t0 = tile * kJoinTile, r0 = t0 + (int64_t)lane * kJoinPerLane;
    const int64_t last = t0 + kJoinTile <= a.np ? t0 + kJoinTile - 1 : a.np - 1;
    kmin = uniform64(a.pkeys[t0]);
    kmax = uniform64(a.pkeys[last]);
    uint32_t valid = 0;
    if (a.vec && t0 + kJoinTile <= a.np) {
        const longlong2 *p = reinterpret_cast<const longlong2 *>(a.pkeys + r0);
        const longlong2 v0 = p[0], v1 = p[1], v2 = p[2], v3 = p[3];
        q[0] = v0.x; q[1] = v0.y; q[2] = v1.x; q[3] = v1.y; q[4] = v2.x; q[5] = v2.y; q[6] = v3.x; q[7] = v3.y;
        valid = 0xffu;
    } else {
#pragma unroll
        for (int k = 0; k < kJoinPerLane; k++) {
            const bool v = r0 + k < a.np;
            q[k] = v ? a.pkeys[r0 + k] : kmax;
            valid |= v ? 1u << k : 0u;
        }
    }
    return valid;
}
__global__ __launch_bounds__(256, 4) void count_merge_mark_kernel(CountMergeArgs a) {
    __shared__ int64_t s_keys[4][kJoinCap];
    const int lane = threadIdx.x & 63;
    int64_t *const sk = s_keys[threadIdx.x >> 6];
    const int64_t ntile = (a.np + kJoinTile - 1) / kJoinTile;
    const int64_t per_xcd = (ntile + 7) / 8, t_begin = (int64_t)(blockIdx.x & 7) * per_xcd;  // (speed only: count_join_kernel)
    const int64_t t_end = t_begin + per_xcd < ntile ? t_begin + per_xcd : ntile;
    const int64_t wave0 = (int64_t)(blockIdx.x >> 3) * 4 + (threadIdx.x >> 6), nwave = (int64_t)(gridDim.x >> 3) * 4;
    for (int64_t tile = t_begin + wave0; tile < t_end; tile += nwave) {
        uint32_t alive = 0;
        if (!a.first) {
            alive = a.flags[tile * 64 + lane];
            if (__ballot(alive != 0) == 0) continue;  // dead since an earlier batch: flags and count stand
        }
        int64_t q[kJoinPerLane], kmin, kmax;
        const uint32_t valid = merge_tile_keys(a, tile, lane, q, kmin, kmax);
        if (a.first) alive = valid;
#pragma unroll 1
        for (int t = 0; t < a.tb.T; t++) {
            if (__ballot(alive != 0) == 0) break;
            const int64_t nk = a.tb.nkeys[t];
            alive &= join_tile_hits(q, kmin, kmax, a.tb.keys[t], nk, a.tb.index[t], (nk + 63) / 64, sk, lane);
        }
        a.flags[tile * 64 + lane] = (uint8_t)alive;
        int cnt = 0;
#pragma unroll
        for (int k = 0; k < kJoinPerLane; k++) cnt += __popcll(__ballot((alive >> k) & 1u));
        if (lane == 0) a.start[tile] = cnt;
    }
}
__global__ __launch_bounds__(256, 4) void count_merge_write_kernel(CountMergeArgs a) {
    __shared__ int64_t s_keys[4][kJoinCap];
    __shared__ int32_t s_vals[4][kJoinCap];
    const int lane = threadIdx.x & 63;
    int64_t *const sk = s_keys[threadIdx.x >> 6];
    int32_t *const sv = s_vals[threadIdx.x >> 6];
    const int64_t ntile = (a.np + kJoinTile - 1) / kJoinTile;
    const int64_t per_xcd = (ntile + 7) / 8, t_begin = (int64_t)(blockIdx.x & 7) * per_xcd;
    const int64_t t_end = t_begin + per_xcd < ntile ? t_begin + per_xcd : ntile;
    const int64_t wave0 = (int64_t)(blockIdx.x >> 3) * 4 + (threadIdx.x >> 6), nwave = (int64_t)(gridDim.x >> 3) * 4;
    const uint64_t below = (1ull << lane) - 1;  // the lanes before this one
    for (int64_t tile = t_begin + wave0; tile < t_end; tile += nwave) {
        const int64_t row0 = uniform64(a.start[tile]);
        if (uniform64(a.start[tile + 1]) == row0) continue;  // nothing kept
        const uint32_t alive = a.flags[tile * 64 + lane];
        int64_t q[kJoinPerLane], kmin, kmax;
        merge_tile_keys(a, tile, lane, q, kmin, kmax);
        int before = 0;  // kept keys of the lanes before this one
#pragma unroll
        for (int k = 0; k < kJoinPerLane; k++) before += __popcll(__ballot((alive >> k) & 1u) & below);
        int64_t row[kJoinPerLane];
#pragma unroll
        for (int k = 0; k < kJoinPerLane; k++) row[k] = row0 + before + __popc(alive & ((1u << k) - 1u));
        if (a.first) {
            const int64_t r0 = tile * kJoinTile + (int64_t)lane * kJoinPerLane;
            int32_t *pc = a.vals_out + (int64_t)a.pcol * a.cap;
#pragma unroll
            for (int k = 0; k < kJoinPerLane; k++)
                if ((alive >> k) & 1u) {
                    a.keys_out[row[k]] = q[k];
                    pc[row[k]] = a.pvals[r0 + k];
                }
        }
#pragma unroll 1
        for (int t = 0; t < a.tb.T; t++) {
            int32_t res[kJoinPerLane];
            const int64_t nk = a.tb.nkeys[t];
            join_tile_table(q, kmin, kmax, a.tb.keys[t], a.tb.vals[t], nk, a.tb.index[t], (nk + 63) / 64, sk, sv, lane, res);
            int32_t *col = a.vals_out + (int64_t)a.col[t] * a.cap;
#pragma unroll
            for (int k = 0; k < kJoinPerLane; k++)
                if ((alive >> k) & 1u) col[row[k]] = res[k];
        }
    }
}
// the scratch of launch_count_merge: the coarse levels of all tables, then the tiles' counts / first rows and their flag bytes
// (+ the scan's own, launch_scan_i64: ru_scan_bytes(ntile))
static size_t count_merge_index_bytes(int S, const int64_t *nkeys) { return (count_join_multi_scratch_bytes(S, nkeys) + 255) / 256 * 256; }
static int64_t count_merge_ntile(int S, const int64_t *nkeys) {
    int64_t np = nkeys[0];
    for (int s = 1; s < S; s++) np = nkeys[s] < np ? nkeys[s] : np;
    return (np + kJoinTile - 1) / kJoinTile;
}
size_t count_merge_scratch_bytes(int S, const int64_t *nkeys) {
    const size_t ntile = (size_t)count_merge_ntile(S, nkeys);
    return count_merge_index_bytes(S, nkeys) + (sizeof(int64_t) * (ntile + 1) + 255) / 256 * 256 + 64 * ntile;
}
// keys / vals / nkeys: host arrays of S entries (device pointers inside), every nkeys[s] >= 1; vals_out: column s at [s * cap], cap >= min nkeys.
// pass 0 = the mark pass, then the caller scans *start_out (ntile + 1 entries, in place), pass 1 = the write pass; n_out = (*start_out)[ntile].
hipError_t launch_count_merge(int pass, int S, const int64_t *const *keys, const int32_t *const *vals, const int64_t *nkeys, int64_t cap,
                              int64_t *keys_out, int32_t *vals_out, void *scratch, int64_t **start_out, int64_t *ntile_out, hipStream_t st) {
    int pivot = 0;
    for (int s = 1; s < S; s++)
        if (nkeys[s] < nkeys[pivot]) pivot = s;
    const int64_t ntile = count_merge_ntile(S, nkeys);
    char *ws = (char *)scratch;
    int64_t *index = (int64_t *)ws;
    int64_t *start = (int64_t *)(ws + count_merge_index_bytes(S, nkeys));
    uint8_t *flags = (uint8_t *)start + (sizeof(int64_t) * (size_t)(ntile + 1) + 255) / 256 * 256;
    *start_out = start;
    *ntile_out = ntile;
    if (pass == 0)
        if (hipError_t e = hipMemsetAsync(start + ntile, 0, sizeof(int64_t), st)) return e;
    int64_t blocks = ((ntile + 3) / 4 + 7) / 8 * 8;  // a multiple of 8: one share of the tiles per XCD
    blocks = blocks > 8192 ? 8192 : blocks;
    int s = 0;
    bool first = true;
    do {  // (S = 1: one launch without tables — every pivot key is kept)
        CountMergeArgs a{};
        a.pkeys = keys[pivot];
        a.pvals = vals[pivot];
        a.np = nkeys[pivot];
        a.pcol = pivot;
        a.first = first ? 1 : 0;
        a.vec = (((uintptr_t)keys[pivot]) & 15) == 0;
        a.flags = flags;
        a.start = start;
        a.cap = cap;
        a.keys_out = keys_out;
        a.vals_out = vals_out;
        int64_t maxidx = 0;
        for (; s < S && a.tb.T < kJoinMaxTables; s++) {
            if (s == pivot) continue;
            const int t = a.tb.T++;
            a.tb.keys[t] = keys[s];
            a.tb.vals[t] = vals[s];
            a.tb.nkeys[t] = nkeys[s];
            a.tb.index[t] = index;
            a.col[t] = s;
            const int64_t nidx = (nkeys[s] + 63) / 64;
            index += nidx + 1;
            maxidx = nidx > maxidx ? nidx : maxidx;
        }
        if (pass == 0) {
            if (a.tb.T > 0) {  // the coarse levels stay for the write pass
                const int64_t bx = (maxidx + 255) / 256;
                join_index_multi_kernel<<<dim3((unsigned)(bx > 1024 ? 1024 : bx), a.tb.T), 256, 0, st>>>(a.tb);
                if (hipError_t e = hipGetLastError()) return e;
            }
            count_merge_mark_kernel<<<(unsigned)blocks, 256, 0, st>>>(a);
        } else {
            count_merge_write_kernel<<<(unsigned)blocks, 256, 0, st>>>(a);
        }
        if (hipError_t e = hipGetLastError()) return e;
        first = false;
        if (s == pivot) s++;  // (the pivot as the last table)
    } while (s < S);
    return hipSuccess;
}

}  // namespace cd
