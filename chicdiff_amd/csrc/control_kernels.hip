// control_kernels.hip — the draws of getControlRegionUniverse (chicdiff.R:430-481) on the device, from a seed: the largest contact per
// chromosome and the number of non-empty regions from the region-level view of RU, one control draw per lane, one sort.  gfx950 only.
//
//   max_contacts, length(unique(regionID)) (:463-466) -> ctrl_contact_kernel: one region per lane, integer maxima per chromosome in LDS
//   sample(bmap$ID), merge, giveDists, giveOneSeed    -> ctrl_draw_kernel: one draw per lane, Philox words from (seed, k, attempt, stream)
//   setkey(baitID, oeID) (:480)                        -> one 64-bit radix sort of (baitID, oeID) keys, then ctrl_unpack_kernel
//
// Every number that leaves a kernel is an integer maximum, a count or a function of (seed, k) alone: arrival order cannot show.  No
// kernel here takes a lock or polls.
#include <math.h>
#include <string.h>

#include <rocprim/rocprim.hpp>

#include "common.h"
#include "devmath.h"
#include "philox.h"
#include "r_rng.h"

namespace cd {

namespace {

constexpr int kCtrlMaxChr = CHICDIFF_CONTROL_MAX_CHR;
constexpr uint32_t kCtrlMaxAttempts = CHICDIFF_CONTROL_MAX_ATTEMPTS;
constexpr uint64_t kCtrlDropped = ~0ull;  // key of a dropped draw: behind every kept one

// signed pairs in unsigned radix order, as candidate_kernels.hip's keys: each half has its sign bit flipped
__device__ __forceinline__ uint64_t ctrl_key(int32_t bait, int32_t oe) {
    return ((uint64_t)((uint32_t)bait ^ 0x80000000u) << 32) | (uint64_t)((uint32_t)oe ^ 0x80000000u);
}

// ---- largest contact per chromosome, number of non-empty regions -----------------------------------------------------------------
// A region's rows are the integers of [minOE, maxOE] that survive the clips, all on one side of its bait (.expandAvoidBait never
// returns a range that straddles the bait), so max |bait - otherEndID| over its rows is max(|bait - minOE|, |bait - maxOE|).  The
// bait's chromosome is the range of IDs that holds it: (lo, hi, code) sorted by lo, disjoint (checked on the host).  A bait in no
// range is not on the map: the merge of :463 drops its rows.  The same grid checks the baitmap's codes.
__global__ __launch_bounds__(256) void ctrl_contact_kernel(const int32_t *__restrict__ ru_bait, int64_t nru, const int64_t *__restrict__ region_ptr,
                                                           const int32_t *__restrict__ minOE, const int32_t *__restrict__ maxOE, int64_t n,
                                                           const int32_t *__restrict__ range_lo, const int32_t *__restrict__ range_hi,
                                                           const int32_t *__restrict__ range_code, int nranges, int nchr,
                                                           const int32_t *__restrict__ bmap_chr, int64_t nb, int32_t *max_contact,
                                                           CtrlResult *res) {
    __shared__ int32_t s_lo[kCtrlMaxChr], s_hi[kCtrlMaxChr], s_code[kCtrlMaxChr], s_max[kCtrlMaxChr];
    __shared__ unsigned int s_count;
    for (int t = threadIdx.x; t < nranges; t += 256) {
        s_lo[t] = range_lo[t];
        s_hi[t] = range_hi[t];
        s_code[t] = range_code[t];
    }
    for (int t = threadIdx.x; t < nchr; t += 256) s_max[t] = 0;
    if (threadIdx.x == 0) s_count = 0;
    __syncthreads();
    const int64_t r = (int64_t)blockIdx.x * 256 + threadIdx.x;
    for (int64_t i = r; i < nb; i += (int64_t)gridDim.x * 256)
        if (bmap_chr[i] >= nchr) atomicMin(&res->bad_bait, (unsigned long long)i);
    bool nonempty = false;
    int32_t code = -1, d = 0;
    if (r < n) {
        const int64_t p0 = region_ptr[r], p1 = region_ptr[r + 1];
        if (p0 < 0 || p1 < p0 || p1 > nru) {
            atomicMin(&res->bad_region, (unsigned long long)r);
        } else if (p1 > p0) {
            nonempty = true;
            const int64_t bait = ru_bait[p0];
            const int64_t a = bait - (int64_t)minOE[r], b = bait - (int64_t)maxOE[r];
            const int64_t m = (a < 0 ? -a : a) > (b < 0 ? -b : b) ? (a < 0 ? -a : a) : (b < 0 ? -b : b);
            d = m > (int64_t)INT32_MAX ? INT32_MAX : (int32_t)m;
            int lo = 0, hi = nranges;  // last range with s_lo <= bait
            while (hi - lo > 1) {
                const int mid = (lo + hi) >> 1;
                if ((int64_t)s_lo[mid] <= bait) lo = mid; else hi = mid;
            }
            if (nranges > 0 && (int64_t)s_lo[lo] <= bait && bait <= (int64_t)s_hi[lo]) code = s_code[lo];
        }
    }
    const bool active = nonempty && code >= 0;
    const uint64_t ne = __ballot(nonempty), act = __ballot(active);
    const int lane = threadIdx.x & 63;
    if (lane == 0 && ne) atomicAdd(&s_count, (unsigned int)__popcll(ne));
    if (act) {
        // neighbouring regions mostly share a chromosome: then one LDS atomic per wave
        const int32_t c0 = __shfl(code, __ffsll((unsigned long long)act) - 1);
        if (__ballot(active && code == c0) == act) {
            int32_t v = active ? d : 0;
            for (int off = 32; off > 0; off >>= 1) {
                const int32_t o = __shfl_xor(v, off);
                v = o > v ? o : v;
            }
            if (lane == 0) atomicMax(&s_max[c0], v);
        } else if (active) {
            atomicMax(&s_max[code], d);
        }
    }
    __syncthreads();
    for (int t = threadIdx.x; t < nchr; t += 256)
        if (s_max[t] > 0) atomicMax(&max_contact[t], s_max[t]);
    if (threadIdx.x == 0 && s_count) atomicAdd(&res->n_regions, (unsigned long long)s_count);
}

// ---- one draw per lane -----------------------------------------------------------------------------------------------------------
// Draw k < n_regions (read from the device: nothing on the host stands between the two kernels); the lanes behind it write the
// dropped key, so that the sort takes all n keys.
__global__ __launch_bounds__(256) void ctrl_draw_kernel(int64_t n, const int32_t *__restrict__ bmap_id, const int32_t *__restrict__ bmap_chr,
                                                        int64_t nb, const int32_t *__restrict__ chr_min, const int32_t *__restrict__ chr_max,
                                                        const int32_t *__restrict__ max_contact, int nchr, uint64_t seed, uint64_t *keys,
                                                        CtrlResult *res) {
    __shared__ int32_t s_min[kCtrlMaxChr], s_max[kCtrlMaxChr];
    __shared__ double s_std[kCtrlMaxChr];  // 0 = no contact on the chromosome
    for (int t = threadIdx.x; t < nchr; t += 256) {
        s_min[t] = chr_min[t];
        s_max[t] = chr_max[t];
        s_std[t] = (double)max_contact[t] / 3.0;  // :472
    }
    __syncthreads();
    const int64_t k = (int64_t)blockIdx.x * 256 + threadIdx.x;
    const bool draw = k < n && (unsigned long long)k < res->n_regions;
    int64_t bait = 0, lo = 0, hi = 0;
    double std = 0.0;
    bool pending = false;
    if (draw) {
        const Philox4 r = control_draw_words(seed, (uint64_t)k, 0, 0);  // stream 0: the bait (:466)
        const uint64_t idx = __umul64hi((uint64_t)r.w[0] | ((uint64_t)r.w[1] << 32), (uint64_t)nb);
        const int32_t c = bmap_chr[idx];
        bait = bmap_id[idx];
        if (c >= 0 && c < nchr && s_std[c] > 0.0) {  // bmap[chr %in% max_contacts$chr] (:468)
            pending = true;
            lo = s_min[c];
            hi = s_max[c];
            std = s_std[c];
        }
    }
    const bool kept = pending;
    int64_t dist = 0;
    for (uint32_t attempt = 0; attempt < kCtrlMaxAttempts; attempt++) {  // giveDists (:434-444), stream 1
        if (!__ballot(pending)) break;
        if (pending) {
            const Philox4 r = control_draw_words(seed, (uint64_t)k, attempt, 1);
            const double z = as241(control_uniform(r.w[0], r.w[1]), FlogFn());
            const int64_t d = (int64_t)rint(z * std);  // R's round(): ties to even
            const int64_t ad = d < 0 ? -d : d;
            if (d != 0 && (bait + ad < hi || bait - ad > lo)) {
                dist = d;
                pending = false;
            }
        }
    }
    if (pending) atomicMin(&res->cap_k, (unsigned long long)k);
    uint64_t key = kCtrlDropped;
    if (kept && !pending) {
        const int64_t fwd = bait + dist;
        const int64_t oe = (fwd < lo || fwd > hi) ? bait - dist : fwd;  // giveOneSeed (:430-432): not strict
        key = ctrl_key((int32_t)bait, (int32_t)oe);
    }
    if (k < n) keys[k] = key;
    const uint64_t kb = __ballot(key != kCtrlDropped);
    if ((threadIdx.x & 63) == 0 && kb) atomicAdd(&res->m, (unsigned long long)__popcll(kb));
}

__global__ __launch_bounds__(256) void ctrl_unpack_kernel(const uint64_t *__restrict__ keys, int64_t n, const CtrlResult *__restrict__ res,
                                                          int32_t *bait, int32_t *oe) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i < n && (unsigned long long)i < res->m) {
        const uint64_t k = keys[i];
        bait[i] = (int32_t)((uint32_t)(k >> 32) ^ 0x80000000u);
        oe[i] = (int32_t)((uint32_t)k ^ 0x80000000u);
    }
}

size_t ctrl_prim_bytes(int64_t n) {
    size_t t = 0;
    uint64_t *k = nullptr;
    (void)rocprim::radix_sort_keys(nullptr, t, k, k, (size_t)n, 0, 64, (hipStream_t)0);
    return t + 256;
}
size_t c256(size_t x) { return (x + 255) & ~(size_t)255; }

}  // namespace

size_t ctrl_workspace_bytes(int64_t n, int32_t nchr) {
    return c256(sizeof(CtrlResult)) + 5 * c256(sizeof(int32_t) * (size_t)nchr) + 2 * c256(sizeof(uint64_t) * (size_t)n) + ctrl_prim_bytes(n);
}

// Everything is enqueued on `st`; *res_out is where the counts and the refusals end up (device memory inside ws).  The five host
// tables (nchr / nranges entries) must stay alive until the stream has been synchronised.
int launch_control_draws(const CtrlArgs &a, const int32_t *range_lo, const int32_t *range_hi, const int32_t *range_code, int nranges, char *ws,
                         hipStream_t st, const CtrlResult **res_out) {
    const int64_t n = a.n;
    const size_t tab = sizeof(int32_t) * (size_t)a.nchr;
    char *q = ws;
    auto take = [&](size_t bytes) { char *r = q; q += c256(bytes); return r; };
    CtrlResult *res = (CtrlResult *)take(sizeof(CtrlResult));
    int32_t *d_min = (int32_t *)take(tab), *d_max = (int32_t *)take(tab);
    int32_t *d_lo = (int32_t *)take(tab), *d_hi = (int32_t *)take(tab), *d_code = (int32_t *)take(tab);
    uint64_t *ka = (uint64_t *)take(8 * (size_t)n), *kb = (uint64_t *)take(8 * (size_t)n);
    void *tmp = q;
    size_t tmp_bytes = ctrl_prim_bytes(n);
    *res_out = res;

    CtrlResult init;
    init.n_regions = init.m = 0;
    init.bad_bait = init.bad_region = init.cap_k = ~0ull;
    if (hipMemcpyAsync(res, &init, sizeof init, hipMemcpyHostToDevice, st) != hipSuccess) return 1;
    if (hipMemcpyAsync(d_min, a.chr_min, tab, hipMemcpyHostToDevice, st) != hipSuccess) return 1;
    if (hipMemcpyAsync(d_max, a.chr_max, tab, hipMemcpyHostToDevice, st) != hipSuccess) return 1;
    if (nranges > 0) {
        const size_t rb = sizeof(int32_t) * (size_t)nranges;
        if (hipMemcpyAsync(d_lo, range_lo, rb, hipMemcpyHostToDevice, st) != hipSuccess) return 1;
        if (hipMemcpyAsync(d_hi, range_hi, rb, hipMemcpyHostToDevice, st) != hipSuccess) return 1;
        if (hipMemcpyAsync(d_code, range_code, rb, hipMemcpyHostToDevice, st) != hipSuccess) return 1;
    }
    if (hipMemsetAsync(a.max_contact, 0, tab, st) != hipSuccess) return 1;
    const unsigned blocks = (unsigned)((n + 255) / 256);
    ctrl_contact_kernel<<<blocks, 256, 0, st>>>(a.ru_bait, a.nru, a.region_ptr, a.minOE, a.maxOE, n, d_lo, d_hi, d_code, nranges, a.nchr,
                                                a.bmap_chr, a.nb, a.max_contact, res);
    ctrl_draw_kernel<<<blocks, 256, 0, st>>>(n, a.bmap_id, a.bmap_chr, a.nb, d_min, d_max, a.max_contact, a.nchr, a.seed, ka, res);
    if (rocprim::radix_sort_keys(tmp, tmp_bytes, ka, kb, (size_t)n, 0, 64, st) != hipSuccess) return 1;
    ctrl_unpack_kernel<<<blocks, 256, 0, st>>>(kb, n, res, a.ctrl_bait, a.ctrl_oe);
    return 0;
}

}  // namespace cd
