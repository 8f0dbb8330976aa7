// candidate_kernels.hip — getCandidateInteractions (chicdiff.R:2068-2163) on the device: the overlap join of the peak matrix's
// rows against the regions of the results table, min(pcol) and the final filter per (baitID, oeID) group, and the pairs of
// the surviving groups in CSR form.  gfx950 only.
//
//   setkey(output, baitID, minOE, maxOE)      -> two stable radix passes over the regions: by maxOE, then by the 64-bit key
//                                                (baitID, minOE); the row index rides along, so ties keep table order
//   the score filter and `delta` (:2082-2127) -> one thread per peak row (cand_peak_pass_kernel), then one sort of (key, row)
//   foverlaps(type = "any", mult = "all")     -> cand_overlap_kernel: sorted peaks against sorted regions
//   by = c("baitID", "oeID") + the filter     -> scans over keep flags and kept degrees, cand_scatter_kernel, cand_fill_kernel
//
// Keys are ordered as SIGNED pairs: each 32-bit half has its sign bit flipped, so the unsigned radix order is the integer order
// data.table sorts by.  Sorts and scans are rocPRIM's; no kernel here takes a lock or polls, and the only atomics raise the
// error words of CandResult (a minimum over row numbers: which row is named does not depend on timing).
#include <math.h>
#include <string.h>

#include <rocprim/rocprim.hpp>

#include "common.h"
#include "devmath.h"

namespace cd {

namespace {

constexpr uint64_t kCandNoKey = ~0ull;  // sort key of a peak row that the score filter drops: behind every selected row
constexpr int kCandWin = 256;           // regions a wave stages in its LDS slice (20 bytes each: 20 KB per workgroup of four waves)
constexpr int kCandRegionBlocks = 1024;
// method = "hmp" (:2135-2137, 2146): 1 + digamma(1) - log(2 / pi), the location of p.hmp's Landau law without its log L; its scale
constexpr double kHmpLoc = 0.874367040387922004, kHmpScale = 1.57079632679489661923;
static __device__ const LandauTable kLandauTable = CD_LANDAU_TABLE_INIT;

__device__ __forceinline__ uint64_t cand_key(int32_t bait, int32_t oe) {
    return ((uint64_t)((uint32_t)bait ^ 0x80000000u) << 32) | (uint64_t)((uint32_t)oe ^ 0x80000000u);
}
__device__ __forceinline__ int32_t cand_key_bait(uint64_t k) { return (int32_t)((uint32_t)(k >> 32) ^ 0x80000000u); }
__device__ __forceinline__ int32_t cand_key_oe(uint64_t k) { return (int32_t)((uint32_t)k ^ 0x80000000u); }
// key of (bait, oe - span): where the look-back for a region that reaches `oe` starts (never in front of the bait's first key)
__device__ __forceinline__ uint64_t cand_key_back(uint64_t k, uint32_t span) {
    int64_t v = (int64_t)cand_key_oe(k) - (int64_t)span;
    if (v < (int64_t)INT32_MIN) v = (int64_t)INT32_MIN;
    return cand_key(cand_key_bait(k), (int32_t)v);
}

// ---- regions: validity, span, first sort key -------------------------------------------------------------------------------------
// foverlaps stops on minOE > maxOE and on NA in a key column: the smallest such row goes to res->bad_region.  span = max(maxOE - minOE)
// over the valid rows: a region that holds fragment oe starts at most `span` fragments in front of it.
__global__ __launch_bounds__(256) void cand_region_pass_kernel(const int32_t *__restrict__ bait, const int32_t *__restrict__ minOE,
                                                               const int32_t *__restrict__ maxOE, int64_t n, uint32_t *k1, int32_t *row,
                                                               uint32_t *span_part, CandResult *res) {
    __shared__ uint32_t s_span[4];
    uint32_t span = 0;
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256) {
        const int32_t b = bait[i], lo = minOE[i], hi = maxOE[i];
        k1[i] = (uint32_t)hi ^ 0x80000000u;
        row[i] = (int32_t)i;
        if (lo > hi || b == INT32_MIN || lo == INT32_MIN) {
            atomicMin(&res->bad_region, (unsigned long long)i);
        } else {
            const uint32_t w = (uint32_t)((int64_t)hi - (int64_t)lo);
            span = w > span ? w : span;
        }
    }
    for (int off = 32; off > 0; off >>= 1) {
        const uint32_t o = __shfl_down(span, off);
        span = o > span ? o : span;
    }
    if ((threadIdx.x & 63) == 0) s_span[threadIdx.x >> 6] = span;
    __syncthreads();
    if (threadIdx.x == 0) {
        for (int w = 1; w < 4; w++) span = s_span[w] > span ? s_span[w] : span;
        span_part[blockIdx.x] = span;
    }
}
__global__ __launch_bounds__(256) void cand_span_kernel(const uint32_t *__restrict__ span_part, int nparts, uint32_t *span_out) {
    __shared__ uint32_t s_span[4];
    uint32_t span = 0;
    for (int i = threadIdx.x; i < nparts; i += 256) span = span_part[i] > span ? span_part[i] : span;
    for (int off = 32; off > 0; off >>= 1) {
        const uint32_t o = __shfl_down(span, off);
        span = o > span ? o : span;
    }
    if ((threadIdx.x & 63) == 0) s_span[threadIdx.x >> 6] = span;
    __syncthreads();
    if (threadIdx.x == 0) {
        for (int w = 1; w < 4; w++) span = s_span[w] > span ? s_span[w] : span;
        *span_out = span;
    }
}
// second sort key, read through the order the first pass left
__global__ __launch_bounds__(256) void cand_region_key_kernel(const int32_t *__restrict__ bait, const int32_t *__restrict__ minOE,
                                                              const int32_t *__restrict__ row, int64_t n, uint64_t *key) {
    for (int64_t j = (int64_t)blockIdx.x * 256 + threadIdx.x; j < n; j += (int64_t)gridDim.x * 256) {
        const int32_t r = row[j];
        key[j] = cand_key(bait[r], minOE[r]);
    }
}

// ---- peaks: the score filter, delta, sort key ------------------------------------------------------------------------------------
// Row sums as double-double (error-free TwoSum, as prep16's column sums): hi + lo is the rounded exact sum whatever the order of the
// columns.  An infinite score breaks the error terms (inf - inf), so the plain sum stands in whenever hi + lo is not finite: it is
// then +-inf or NaN, as R's.
struct CandDD { double hi = 0.0, lo = 0.0, plain = 0.0; };
__device__ __forceinline__ void cand_dd_add(CandDD &a, double x) {
    const double s = a.hi + x, bb = s - a.hi;
    a.lo += (a.hi - (s - bb)) + (x - bb);
    a.hi = s;
    a.plain += x;
}
__device__ __forceinline__ double cand_dd_value(const CandDD &a) {
    const double t = a.hi + a.lo;
    return (t - t == 0.0) ? t : a.plain;
}
__global__ __launch_bounds__(256) void cand_peak_pass_kernel(const int32_t *__restrict__ pbait, const int32_t *__restrict__ poe,
                                                             const double *__restrict__ scores, int64_t P, int ncols, int ncond1, int merged,
                                                             double score, uint64_t *key, int32_t *row, double *delta, CandResult *res) {
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < P; i += (int64_t)gridDim.x * 256) {
        CandDD s1, s2;
        bool sel = false;
        double nxt = scores[i];
        for (int c = 0; c < ncols; c++) {
            const double cur = nxt;
            if (c + 1 < ncols) nxt = scores[(int64_t)(c + 1) * P + i];  // in flight while this column is summed
            sel |= cur > score;                                         // NA never passes (:2085)
            if (c < ncond1) cand_dd_add(s1, cur); else cand_dd_add(s2, cur);
        }
        double d;
        if (merged) {
            d = fabs(s2.plain - s1.plain);  // :2126 — the scores themselves, NO asinh
        } else {
            const double m1 = cand_dd_value(s1) / (double)ncond1, m2 = cand_dd_value(s2) / (double)(ncols - ncond1);
            d = fabs(asinh(m1) - asinh(m2));
        }
        const uint64_t k = cand_key(pbait[i], poe[i]);
        if (sel && k == kCandNoKey) atomicMin(&res->bad_peak_key, (unsigned long long)i);
        key[i] = sel ? k : kCandNoKey;
        row[i] = (int32_t)i;
        delta[i] = d;
    }
}

// ---- the overlap join ------------------------------------------------------------------------------------------------------------
// first index in [lo, hi) whose key is >= k (UPPER: > k)
template <bool UPPER, class Keys>
__device__ __forceinline__ int64_t cand_bound(const Keys &keys, int64_t lo, int64_t hi, uint64_t k) {
    while (lo < hi) {
        const int64_t mid = lo + ((hi - lo) >> 1);
        const uint64_t v = keys[mid];
        if (UPPER ? v <= k : v < k) lo = mid + 1; else hi = mid;
    }
    return lo;
}
// A wave owns 64 consecutive sorted peaks.  Its regions lie in ONE window of the sorted region table,
// [lower_bound(first key - span), upper_bound(last key)): found once, staged as (key, maxOE, p) in the wave's LDS slice when it
// fits — one bait with thousands of regions is legal, then the lanes search global memory instead.  Each lane then scans
// [lower_bound(bait, oe - span), upper_bound(bait, oe)) and tests maxOE >= oe.  The look-back by span is what finds a wide region
// that sits many rows in front of the peak's neighbours in key order.
// Per sorted peak: keep flag, kept degree (the two scan inputs), the combined p, and for the fill the scan's first index and which
// of its first 64 candidates matched.
// METHOD: CHICDIFF_CAND_MIN — the minimum of p over the matches, NA if one is NA; CHICDIFF_CAND_HMP — p.hmp of the matches: NA and
// p > 1 count as 1 (:2136), the reciprocals are summed in match (= pair) order, each a division, and the sum goes through
// landau_tail once per peak.  Only the reduction differs: the scan, its order and everything written for the fill are shared.
template <int METHOD>
__global__ __launch_bounds__(256) void cand_overlap_kernel(const uint64_t *__restrict__ pkey, const int32_t *__restrict__ prow, int64_t P,
                                                           const double *__restrict__ delta, const uint64_t *__restrict__ rkey,
                                                           const int32_t *__restrict__ rrow, int64_t n, const int32_t *__restrict__ maxOE,
                                                           const double *__restrict__ p, const uint32_t *__restrict__ span_p, double pvcut,
                                                           double min_delta, int32_t *keep, int64_t *kdeg, double *minp, int32_t *first,
                                                           uint64_t *mask, CandResult *res) {
    __shared__ uint64_t s_key[4][kCandWin];
    __shared__ double s_p[4][kCandWin];
    __shared__ int32_t s_max[4][kCandWin];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int64_t s = ((int64_t)blockIdx.x * 4 + wave) * 64 + lane;
    const bool in = s < P;
    const uint64_t key = in ? pkey[s] : kCandNoKey;
    const bool sel = key != kCandNoKey;
    const int nsel = __popcll(__ballot(sel));  // the selected rows are a prefix of the wave: the dropped ones sort last
    uint64_t prev = __shfl_up(key, 1);
    if (lane == 0) prev = s > 0 && in ? pkey[s - 1] : kCandNoKey;
    if (nsel == 0) {
        if (in) { keep[s] = 0; kdeg[s] = 0; }
        return;
    }
    const uint32_t span = *span_p;
    const uint64_t kfirst = __shfl(key, 0), klast = __shfl(key, nsel - 1);
    const int64_t wlo = cand_bound<false>(rkey, (int64_t)0, n, cand_key_back(kfirst, span));
    const int64_t whi = cand_bound<true>(rkey, wlo, n, klast);
    const int W = whi - wlo <= kCandWin ? (int)(whi - wlo) : -1;  // -1: not staged
    for (int j = lane; j < W; j += 64) {
        const int32_t r = rrow[wlo + j];
        s_key[wave][j] = rkey[wlo + j];
        s_max[wave][j] = maxOE[r];
        s_p[wave][j] = p[r];
    }
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
    if (!sel) {
        if (in) { keep[s] = 0; kdeg[s] = 0; }
        return;
    }
    const int32_t oe = cand_key_oe(key);
    const uint64_t kback = cand_key_back(key, span);
    int64_t a, b;  // relative to wlo
    if (W >= 0) {
        const uint64_t *sk = s_key[wave];
        a = cand_bound<false>(sk, (int64_t)0, (int64_t)W, kback);
        b = cand_bound<true>(sk, a, (int64_t)W, key);
    } else {
        a = cand_bound<false>(rkey, wlo, whi, kback) - wlo;
        b = cand_bound<true>(rkey, wlo + a, whi, key) - wlo;
    }
    int32_t deg = 0;
    double m = METHOD == CHICDIFF_CAND_HMP ? 0.0 : INFINITY;  // hmp: the sum of 1 / p'
    bool na = false;
    uint64_t msk = 0;
    for (int64_t j = a; j < b; j++) {
        int32_t mx;
        double pv;
        if (W >= 0) {
            mx = s_max[wave][j];
            pv = s_p[wave][j];
        } else {
            const int32_t r = rrow[wlo + j];
            mx = maxOE[r];
            pv = p[r];
        }
        if (mx >= oe) {
            deg++;
            if constexpr (METHOD == CHICDIFF_CAND_HMP) {
                m += 1.0 / (pv <= 1.0 ? pv : 1.0);  // NA fails the comparison too
            } else {
                na |= pv != pv;       // min() without na.rm: one NA makes the minimum NA (fmin would drop it)
                m = pv < m ? pv : m;
            }
            if (j - a < 64) msk |= 1ull << (j - a);
        }
    }
    double mp;
    if constexpr (METHOD == CHICDIFF_CAND_HMP) {
        const double L = (double)deg;  // x = mean of 1 / p' >= 1, so z > -14 for every L < 2^31; p = 0 gives x = z = inf and 0
        mp = deg > 0 ? landau_tail((m / L - (flog(L) + kHmpLoc)) / kHmpScale, kLandauTable) : NAN;
    } else {
        mp = na ? NAN : m;
    }
    const int32_t r = prow[s];
    const bool kp = deg > 0 && mp <= pvcut && delta[r] >= min_delta;  // a NaN on either side drops the group (:2161)
    if (prev == key) atomicMin(&res->dup_peak, (unsigned long long)r);  // two selected rows with one (baitID, oeID)
    keep[s] = kp ? 1 : 0;
    kdeg[s] = kp ? (int64_t)deg : 0;
    minp[s] = mp;
    first[s] = (int32_t)(wlo + a);
    mask[s] = msk;
}

// ---- compaction and fill -----------------------------------------------------------------------------------------------------------
// slot / ptr: exclusive scans of keep / kdeg over P + 1 entries (entry P = 0), so entry P holds the totals
__global__ __launch_bounds__(256) void cand_scatter_kernel(const uint64_t *__restrict__ pkey, const int32_t *__restrict__ prow, int64_t P,
                                                           const double *__restrict__ delta, const int32_t *__restrict__ keep,
                                                           const int32_t *__restrict__ slot, const int64_t *__restrict__ ptr,
                                                           const double *__restrict__ minp, const int32_t *__restrict__ first,
                                                           const uint64_t *__restrict__ mask, int32_t *group_peak, int64_t *group_ptr,
                                                           double *group_min_p, double *group_delta, int32_t *g_first, uint64_t *g_mask,
                                                           int32_t *g_oe, CandResult *res) {
    for (int64_t s = (int64_t)blockIdx.x * 256 + threadIdx.x; s <= P; s += (int64_t)gridDim.x * 256) {
        if (s == P) {
            group_ptr[slot[P]] = ptr[P];
            res->ngroups = slot[P];
            res->npairs = ptr[P];
        } else if (keep[s]) {
            const int32_t g = slot[s], r = prow[s];
            group_peak[g] = r;
            group_ptr[g] = ptr[s];
            group_min_p[g] = minp[s];
            group_delta[g] = delta[r];
            g_first[g] = first[s];
            g_mask[g] = mask[s];
            g_oe[g] = cand_key_oe(pkey[s]);
        }
    }
}
// Pair rows are written by consecutive threads (coalesced), as ru_fill_kernel's: a workgroup owns 256 groups, keeps their CSR
// offsets in LDS, and each pair finds its group by binary search there.  The k-th region of a group is the k-th set bit of the
// group's match mask; only a group that scanned more than 64 candidates walks on from the 65th.  Nothing is written when the
// pairs do not fit (the host reports the need).
__global__ __launch_bounds__(256) void cand_fill_kernel(const CandResult *__restrict__ res, int64_t capacity, const int64_t *__restrict__ group_ptr,
                                                        const int32_t *__restrict__ g_first, const uint64_t *__restrict__ g_mask,
                                                        const int32_t *__restrict__ g_oe, const int32_t *__restrict__ rrow, int64_t n,
                                                        const int32_t *__restrict__ maxOE, int32_t *pair_row) {
    __shared__ int64_t s_ptr[257];
    __shared__ uint64_t s_mask[256];
    __shared__ int32_t s_first[256], s_oe[256];
    const int64_t ngroups = res->ngroups;
    if (res->npairs > capacity) return;
    for (int64_t g0 = (int64_t)blockIdx.x * 256; g0 < ngroups; g0 += (int64_t)gridDim.x * 256) {
        const int ng = ngroups - g0 < 256 ? (int)(ngroups - g0) : 256;
        __syncthreads();
        if ((int)threadIdx.x < ng) {
            s_ptr[threadIdx.x] = group_ptr[g0 + threadIdx.x];
            s_mask[threadIdx.x] = g_mask[g0 + threadIdx.x];
            s_first[threadIdx.x] = g_first[g0 + threadIdx.x];
            s_oe[threadIdx.x] = g_oe[g0 + threadIdx.x];
        }
        if (threadIdx.x == 0) s_ptr[ng] = group_ptr[g0 + ng];
        __syncthreads();
        const int64_t r1 = s_ptr[ng];
        for (int64_t r = s_ptr[0] + threadIdx.x; r < r1; r += 256) {
            int a = 0, e = ng;  // last group with s_ptr[a] <= r
            while (e - a > 1) {
                const int mid = (a + e) >> 1;
                if (s_ptr[mid] <= r) a = mid; else e = mid;
            }
            int64_t k = r - s_ptr[a];
            uint64_t m = s_mask[a];
            const int c = __popcll(m);
            int64_t j = s_first[a];
            if (k < c) {
                for (int q = 0; q < (int)k; q++) m &= m - 1ull;  // drop the k lowest set bits
                j += __ffsll((unsigned long long)m) - 1;
            } else {
                k -= c;
                const int32_t oe = s_oe[a];
                for (j += 64; j < n; j++)
                    if (maxOE[rrow[j]] >= oe && k-- == 0) break;
            }
            if (j < n) pair_row[r] = rrow[j];
        }
    }
}

// out[i] = landau_tail(z[i]) as cand_overlap_kernel<CHICDIFF_CAND_HMP> calls it
__global__ __launch_bounds__(256) void landau_selftest_kernel(const double *__restrict__ z, int64_t n, double *out) {
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256) out[i] = landau_tail(z[i], kLandauTable);
}

int cand_grid(int64_t items) {
    int64_t b = (items + 255) / 256;
    return (int)(b < 1 ? 1 : (b > 4096 ? 4096 : b));
}
// sizes of rocPRIM's temporary storage: the largest of the sorts and scans below
size_t cand_prim_bytes(int64_t n, int64_t P) {
    size_t need = 0, t = 0;
    uint32_t *k32 = nullptr;
    uint64_t *k64 = nullptr;
    int32_t *v = nullptr;
    int64_t *l = nullptr;
    (void)rocprim::radix_sort_pairs(nullptr, t, k32, k32, v, v, (size_t)n, 0, 32, (hipStream_t)0);
    need = t > need ? t : need;
    (void)rocprim::radix_sort_pairs(nullptr, t, k64, k64, v, v, (size_t)(n > P ? n : P), 0, 64, (hipStream_t)0);
    need = t > need ? t : need;
    (void)rocprim::exclusive_scan(nullptr, t, l, l, (int64_t)0, (size_t)P + 1, rocprim::plus<int64_t>(), (hipStream_t)0);
    need = t > need ? t : need;
    (void)rocprim::exclusive_scan(nullptr, t, v, v, (int32_t)0, (size_t)P + 1, rocprim::plus<int32_t>(), (hipStream_t)0);
    need = t > need ? t : need;
    return need + 256;
}
size_t a256(size_t x) { return (x + 255) & ~(size_t)255; }

}  // namespace

size_t cand_workspace_bytes(int64_t n, int64_t P) {
    const size_t N = (size_t)n, Q = (size_t)P + 1;
    return a256(sizeof(CandResult)) + a256(4 * kCandRegionBlocks) + 2 * a256(4 * N) /* k1 */ + 2 * a256(4 * N) /* rows */ + 2 * a256(8 * N) /* keys */ +
           2 * a256(8 * Q) /* peak keys */ + 2 * a256(4 * Q) /* peak rows */ + a256(8 * Q) /* delta */ + 2 * a256(4 * Q) /* keep, slot */ +
           2 * a256(8 * Q) /* kdeg, ptr */ + a256(8 * Q) /* minp */ + 2 * a256(4 * Q) /* first */ + 2 * a256(8 * Q) /* mask */ + a256(4 * Q) /* oe */ +
           cand_prim_bytes(n, P);
}

// Everything is enqueued on `st`; *res_out is where the two counts and the three error words end up (device memory inside ws).
int launch_candidates(const CandArgs &a, char *ws, hipStream_t st, const CandResult **res_out) {
    const int64_t n = a.n, P = a.npeaks;
    const size_t N = (size_t)n, Q = (size_t)P + 1;
    char *q = ws;
    auto take = [&](size_t bytes) { char *r = q; q += a256(bytes); return r; };
    CandResult *res = (CandResult *)take(sizeof(CandResult));
    uint32_t *span_part = (uint32_t *)take(4 * (kCandRegionBlocks - 1));
    uint32_t *span = span_part + (kCandRegionBlocks - 1);
    uint32_t *k1a = (uint32_t *)take(4 * N), *k1b = (uint32_t *)take(4 * N);
    int32_t *ra = (int32_t *)take(4 * N), *rb = (int32_t *)take(4 * N);
    uint64_t *ka = (uint64_t *)take(8 * N), *kb = (uint64_t *)take(8 * N);
    uint64_t *pka = (uint64_t *)take(8 * Q), *pkb = (uint64_t *)take(8 * Q);
    int32_t *pra = (int32_t *)take(4 * Q), *prb = (int32_t *)take(4 * Q);
    double *delta = (double *)take(8 * Q);
    int32_t *keep = (int32_t *)take(4 * Q), *slot = (int32_t *)take(4 * Q);
    int64_t *kdeg = (int64_t *)take(8 * Q), *ptr = (int64_t *)take(8 * Q);
    double *minp = (double *)take(8 * Q);
    int32_t *first = (int32_t *)take(4 * Q), *g_first = (int32_t *)take(4 * Q);
    uint64_t *mask = (uint64_t *)take(8 * Q), *g_mask = (uint64_t *)take(8 * Q);
    int32_t *g_oe = (int32_t *)take(4 * Q);
    void *tmp = q;
    size_t tmp_bytes = cand_prim_bytes(n, P);
    *res_out = res;

    CandResult init;
    init.bad_region = init.bad_peak_key = init.dup_peak = ~0ull;
    init.ngroups = init.npairs = 0;
    if (hipMemcpyAsync(res, &init, sizeof init, hipMemcpyHostToDevice, st) != hipSuccess) return 1;
    if (hipMemsetAsync(a.group_ptr, 0, sizeof(int64_t), st) != hipSuccess) return 1;
    if (P == 0) return 0;
    if (hipMemsetAsync(keep + P, 0, sizeof(int32_t), st) != hipSuccess) return 1;
    if (hipMemsetAsync(kdeg + P, 0, sizeof(int64_t), st) != hipSuccess) return 1;

    // regions: stable order by (baitID, minOE, maxOE, row)
    const int rblocks = cand_grid(n) < kCandRegionBlocks - 1 ? cand_grid(n) : kCandRegionBlocks - 1;
    cand_region_pass_kernel<<<rblocks, 256, 0, st>>>(a.bait, a.minOE, a.maxOE, n, k1a, ra, span_part, res);
    cand_span_kernel<<<1, 256, 0, st>>>(span_part, rblocks, span);
    size_t t = tmp_bytes;
    if (rocprim::radix_sort_pairs(tmp, t, k1a, k1b, ra, rb, N, 0, 32, st) != hipSuccess) return 1;
    cand_region_key_kernel<<<cand_grid(n), 256, 0, st>>>(a.bait, a.minOE, rb, n, ka);
    t = tmp_bytes;
    if (rocprim::radix_sort_pairs(tmp, t, ka, kb, rb, ra, N, 0, 64, st) != hipSuccess) return 1;
    // peaks
    cand_peak_pass_kernel<<<cand_grid(P), 256, 0, st>>>(a.peak_bait, a.peak_oe, a.scores, P, a.ncols, a.ncond1, a.merged, a.score, pka, pra,
                                                       delta, res);
    t = tmp_bytes;
    if (rocprim::radix_sort_pairs(tmp, t, pka, pkb, pra, prb, (size_t)P, 0, 64, st) != hipSuccess) return 1;
    // join, compaction, fill
    if (a.method == CHICDIFF_CAND_HMP)
        cand_overlap_kernel<CHICDIFF_CAND_HMP><<<(unsigned)((P + 255) / 256), 256, 0, st>>>(pkb, prb, P, delta, kb, ra, n, a.maxOE, a.p, span, a.pvcut,
                                                                                           a.min_delta, keep, kdeg, minp, first, mask, res);
    else
        cand_overlap_kernel<CHICDIFF_CAND_MIN><<<(unsigned)((P + 255) / 256), 256, 0, st>>>(pkb, prb, P, delta, kb, ra, n, a.maxOE, a.p, span, a.pvcut,
                                                                                           a.min_delta, keep, kdeg, minp, first, mask, res);
    t = tmp_bytes;
    if (rocprim::exclusive_scan(tmp, t, keep, slot, (int32_t)0, Q, rocprim::plus<int32_t>(), st) != hipSuccess) return 1;
    t = tmp_bytes;
    if (rocprim::exclusive_scan(tmp, t, kdeg, ptr, (int64_t)0, Q, rocprim::plus<int64_t>(), st) != hipSuccess) return 1;
    cand_scatter_kernel<<<cand_grid(P + 1), 256, 0, st>>>(pkb, prb, P, delta, keep, slot, ptr, minp, first, mask, a.group_peak, a.group_ptr,
                                                         a.group_min_p, a.group_delta, g_first, g_mask, g_oe, res);
    cand_fill_kernel<<<cand_grid(P), 256, 0, st>>>(res, a.pair_capacity, a.group_ptr, g_first, g_mask, g_oe, ra, n, a.maxOE, a.pair_row);
    return 0;
}

void launch_landau_selftest(const double *z, int64_t n, double *out, hipStream_t st) {
    landau_selftest_kernel<<<cand_grid(n), 256, 0, st>>>(z, n, out);
}

}  // namespace cd
