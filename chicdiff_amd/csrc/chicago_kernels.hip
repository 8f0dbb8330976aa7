// chicago_kernels.hip — the Chicago background tables of one replicate (chicdiff.R:656-692, 538-548) on the device: first s_j / tblb
// per bait, first s_i / tlb per other end, Tmean of every (tblb, tlb) pair, refBinMean per distbin.  gfx950 only.  No sort.
//
// WINNER RULE.  Every "first" of the reference follows setkey(x, baitID, otherEndID), a stable sort, so it is the row that
// minimises (baitID, otherEndID, row) within its group — a minimum of integers, whatever the order of the rows, the launch shape or
// the arrival order of the atomics:
//   per bait        the bait half of the key is constant: one 64-bit atomicMin of (otherEndID << 32 | row) into the bait's slot
//   per other end   likewise (baitID << 32 | row) into the other end's slot
//   per (tblb, tlb) the full key (baitID << 32 | otherEndID) may repeat: pass 1 finds the smallest key, pass 2 the smallest row
//                   among the rows that carry it
//   per distbin     min and max of an order-preserving image of the refBinMean bits: equal = one value, the distance function's input
// IDs are signed (each 32-bit half has its sign bit flipped, as candidate_kernels.hip's keys); rows are < 2^32.
//
//   chicago_init_kernel      slots to all ones, outputs to NaN / -1
//   chicago_pass1_kernel     streams bait, oe, tblb, tlb, distbin, refBinMean (28 bytes a row): the two slot minima in global memory
//                            (L2-resident: 16 nid bytes), the pair and distbin tables private per workgroup in LDS, merged once
//   chicago_pass2_kernel     streams bait, oe, tblb, tlb (16 bytes a row): the row whose packed word IS its slot writes the two
//                            values of its fragment (one writer per cell); rows that carry their pair's smallest key take part in a
//                            minimum over the row number
//   chicago_epilogue_kernel  one thread per pair and per distbin code
//
// Chicago tables arrive keyed by bait, so consecutive lanes aim at ONE bait slot: runs of equal slots are merged inside the wave
// by a segmented minimum over neighbouring lanes, and only a run's first lane issues the global atomic.  Switching that off
// (option "chicago_tables_run_merge") changes no result: a minimum does not care how often it is taken.
#include <math.h>

#include "common.h"

namespace cd {

namespace {

constexpr uint64_t kNone = ~0ull;
constexpr int kRowsPerLane = CHICDIFF_CHICAGO_ROWS_PER_WORKGROUP / 256;
static_assert(CHICDIFF_CHICAGO_ROWS_PER_WORKGROUP % 256 == 0, "a workgroup takes whole tiles of 256 rows");

__device__ __forceinline__ uint32_t flip(int32_t v) { return (uint32_t)v ^ 0x80000000u; }
// doubles (no NaN) -> unsigned integers in the same order
__device__ __forceinline__ uint64_t ordered_bits(double x) {
    const uint64_t u = (uint64_t)__double_as_longlong(x);
    return (u >> 63) ? ~u : (u | 0x8000000000000000ull);
}
__device__ __forceinline__ double ordered_value(uint64_t u) {
    return __longlong_as_double((long long)((u >> 63) ? (u & 0x7fffffffffffffffull) : ~u));
}

// v of every lane -> the minimum over the lanes from this one to the end of its run (runs: maximal stretches of neighbouring lanes
// with one slot; head = this lane starts one).  A wave without two equal neighbours skips the six steps.
__device__ __forceinline__ uint64_t run_min(uint64_t v, int64_t slot, int lane, bool &head) {
    const int64_t prev = __shfl_up(slot, 1);
    head = lane == 0 || prev != slot;
    const unsigned long long heads = __ballot(head);
    if (heads == ~0ull) return v;
    const unsigned long long later = lane == 63 ? 0ull : heads >> (lane + 1);
    const int left = later ? __ffsll(later) : 64 - lane;  // lanes of the run from this one on
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) {
        const uint64_t o = __shfl_down(v, off);
        if (off < left && o < v) v = o;
    }
    return v;
}

__global__ __launch_bounds__(256) void chicago_init_kernel(uint64_t *bait_slot, uint64_t *oe_slot, int32_t nid, uint64_t *pair_key,
                                                           uint32_t *pair_row, int32_t npairs, uint64_t *db_min, uint64_t *db_max, int32_t ndb,
                                                           uint32_t *status, double *sj, double *si, int32_t *tblb_of, int32_t *tlb_of) {
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < nid; i += (int64_t)gridDim.x * 256) {
        bait_slot[i] = kNone;
        oe_slot[i] = kNone;
        sj[i] = NAN;
        si[i] = NAN;
        tblb_of[i] = -1;
        tlb_of[i] = -1;
    }
    if (blockIdx.x == 0) {
        for (int i = threadIdx.x; i < npairs; i += 256) {
            pair_key[i] = kNone;
            pair_row[i] = 0xffffffffu;
        }
        for (int i = threadIdx.x; i < ndb; i += 256) {
            db_min[i] = kNone;
            db_max[i] = 0ull;
        }
        if (threadIdx.x == 0) *status = 0u;
    }
}

// the (tblb, tlb) cell of a row, -1 when either code is NA; a code outside [-1, levels) raises the status word's second bit
__device__ __forceinline__ int pair_of(int32_t tb, int32_t tl, int32_t ntblb, int32_t ntlb, bool &bad) {
    bad |= tb < -1 || tb >= ntblb || tl < -1 || tl >= ntlb;
    return (tb < 0 || tl < 0 || tb >= ntblb || tl >= ntlb) ? -1 : tb * ntlb + tl;
}

__global__ __launch_bounds__(256) void chicago_pass1_kernel(const int32_t *__restrict__ bait, const int32_t *__restrict__ oe,
                                                            const int32_t *__restrict__ tblb, const int32_t *__restrict__ tlb,
                                                            const int32_t *__restrict__ distbin, const double *__restrict__ ref, int64_t n,
                                                            int32_t id_min, int32_t nid, int32_t ntblb, int32_t ntlb, int32_t ndistbin,
                                                            int merge, uint64_t *bait_slot, uint64_t *oe_slot, uint64_t *pair_key,
                                                            uint64_t *db_min, uint64_t *db_max, uint32_t *status) {
    __shared__ uint64_t s_pair[CHICDIFF_CHICAGO_MAX_PAIRS];
    __shared__ uint64_t s_min[CHICDIFF_CHICAGO_MAX_DISTBIN + 1], s_max[CHICDIFF_CHICAGO_MAX_DISTBIN + 1];
    const int npairs = ntblb * ntlb, ndb = ndistbin + 1, lane = threadIdx.x & 63;
    for (int i = threadIdx.x; i < npairs; i += 256) s_pair[i] = kNone;
    for (int i = threadIdx.x; i < ndb; i += 256) {
        s_min[i] = kNone;
        s_max[i] = 0ull;
    }
    __syncthreads();
    const int64_t base = (int64_t)blockIdx.x * CHICDIFF_CHICAGO_ROWS_PER_WORKGROUP;
    bool bad = false;
#pragma unroll 4
    for (int it = 0; it < kRowsPerLane; it++) {
        const int64_t r = base + (int64_t)it * 256 + threadIdx.x;
        if (base + (int64_t)it * 256 >= n) break;  // (the whole workgroup)
        const bool in = r < n;
        int32_t b = 0, o = 0, tb = -1, tl = -1, db = -1;
        double x = NAN;
        if (in) {
            b = bait[r]; o = oe[r]; tb = tblb[r]; tl = tlb[r]; db = distbin[r]; x = ref[r];
        }
        const int64_t bs = (int64_t)b - id_min, os = (int64_t)o - id_min;
        const int64_t bslot = in && bs >= 0 && bs < nid ? bs : -1, oslot = in && os >= 0 && os < nid ? os : -1;
        uint64_t bv = ((uint64_t)flip(o) << 32) | (uint32_t)r, ov = ((uint64_t)flip(b) << 32) | (uint32_t)r;
        bool bhead = true, ohead = true;
        if (merge) {
            bv = run_min(bv, bslot, lane, bhead);
            ov = run_min(ov, oslot, lane, ohead);
        }
        if (bhead && bslot >= 0) atomicMin((unsigned long long *)&bait_slot[bslot], (unsigned long long)bv);
        if (ohead && oslot >= 0) atomicMin((unsigned long long *)&oe_slot[oslot], (unsigned long long)ov);
        const int p = pair_of(tb, tl, ntblb, ntlb, bad);
        if (p >= 0) atomicMin((unsigned long long *)&s_pair[p], (unsigned long long)(((uint64_t)flip(b) << 32) | flip(o)));
        bad |= db < -1 || db >= ndistbin;
        if (x == x && db >= -1 && db < ndistbin) {  // an NA distbin is a value of its own: the last entry
            const int d = db < 0 ? ndistbin : db;
            const uint64_t u = ordered_bits(x);
            atomicMin((unsigned long long *)&s_min[d], (unsigned long long)u);
            atomicMax((unsigned long long *)&s_max[d], (unsigned long long)u);
        }
    }
    __syncthreads();
    for (int i = threadIdx.x; i < npairs; i += 256)
        if (s_pair[i] != kNone) atomicMin((unsigned long long *)&pair_key[i], (unsigned long long)s_pair[i]);
    for (int i = threadIdx.x; i < ndb; i += 256)
        if (s_min[i] != kNone) {
            atomicMin((unsigned long long *)&db_min[i], (unsigned long long)s_min[i]);
            atomicMax((unsigned long long *)&db_max[i], (unsigned long long)s_max[i]);
        }
    if (bad) atomicOr(status, (unsigned int)CHICDIFF_CHICAGO_BAD_CODE);
}

__global__ __launch_bounds__(256) void chicago_pass2_kernel(const int32_t *__restrict__ bait, const int32_t *__restrict__ oe,
                                                            const int32_t *__restrict__ tblb, const int32_t *__restrict__ tlb,
                                                            const double *__restrict__ s_j, const double *__restrict__ s_i, int64_t n,
                                                            int32_t id_min, int32_t nid, int32_t ntblb, int32_t ntlb,
                                                            const uint64_t *__restrict__ bait_slot, const uint64_t *__restrict__ oe_slot,
                                                            const uint64_t *__restrict__ pair_key, uint32_t *pair_row, double *sj, double *si,
                                                            int32_t *tblb_of, int32_t *tlb_of) {
    __shared__ uint64_t s_key[CHICDIFF_CHICAGO_MAX_PAIRS];
    __shared__ uint32_t s_row[CHICDIFF_CHICAGO_MAX_PAIRS];
    const int npairs = ntblb * ntlb;
    for (int i = threadIdx.x; i < npairs; i += 256) {
        s_key[i] = pair_key[i];
        s_row[i] = 0xffffffffu;
    }
    __syncthreads();
    const int64_t base = (int64_t)blockIdx.x * CHICDIFF_CHICAGO_ROWS_PER_WORKGROUP;
    bool bad = false;  // (reported by pass 1)
#pragma unroll 4
    for (int it = 0; it < kRowsPerLane; it++) {
        const int64_t r = base + (int64_t)it * 256 + threadIdx.x;
        if (r >= n) break;
        const int32_t b = bait[r], o = oe[r], tb = tblb[r], tl = tlb[r];
        const int64_t bs = (int64_t)b - id_min, os = (int64_t)o - id_min;
        if (bs >= 0 && bs < nid && bait_slot[bs] == (((uint64_t)flip(o) << 32) | (uint32_t)r)) {  // the bait's winner: kept even when NA
            sj[bs] = s_j[r];
            tblb_of[bs] = tb >= 0 && tb < ntblb ? tb : -1;
        }
        if (os >= 0 && os < nid && oe_slot[os] == (((uint64_t)flip(b) << 32) | (uint32_t)r)) {
            si[os] = s_i[r];
            tlb_of[os] = tl >= 0 && tl < ntlb ? tl : -1;
        }
        const int p = pair_of(tb, tl, ntblb, ntlb, bad);
        if (p >= 0 && s_key[p] == (((uint64_t)flip(b) << 32) | flip(o))) atomicMin(&s_row[p], (uint32_t)r);
    }
    __syncthreads();
    for (int i = threadIdx.x; i < npairs; i += 256)
        if (s_row[i] != 0xffffffffu) atomicMin(&pair_row[i], s_row[i]);
}

__global__ __launch_bounds__(256) void chicago_epilogue_kernel(const double *__restrict__ Tmean, const uint32_t *__restrict__ pair_row,
                                                               int32_t npairs, const uint64_t *__restrict__ db_min,
                                                               const uint64_t *__restrict__ db_max, int32_t ndb, double *T, double *ref_out,
                                                               uint32_t *status) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i < npairs) {
        const uint32_t r = pair_row[i];
        T[i] = r != 0xffffffffu ? Tmean[r] : NAN;  // (n < 2^32 - 1 rows: all ones is no row)
    } else if (i < npairs + ndb) {
        const int d = i - npairs;
        const uint64_t lo = db_min[d], hi = db_max[d];
        double v = NAN;
        if (lo != kNone) {
            if (lo == hi) v = ordered_value(lo);
            else atomicOr(status, (unsigned int)CHICDIFF_CHICAGO_NOT_A_FUNCTION);  // two refBinMean values under one distbin
        }
        ref_out[d] = v;
    }
}

size_t a256(size_t x) { return (x + 255) & ~(size_t)255; }

}  // namespace

size_t chicago_workspace_bytes(int32_t nid) {
    return a256(256) + 2 * a256(8 * (size_t)nid) + a256(8 * CHICDIFF_CHICAGO_MAX_PAIRS) + a256(4 * CHICDIFF_CHICAGO_MAX_PAIRS) +
           2 * a256(8 * (CHICDIFF_CHICAGO_MAX_DISTBIN + 1));
}

// stage 0: init, 1: pass 1, 2: pass 2 + epilogue (the caller brackets each with a timer); *status_out: the device status word inside ws
void launch_chicago_tables(const ChicagoArgs &a, int stage, int merge, char *ws, hipStream_t st, const uint32_t **status_out) {
    char *q = ws;
    auto take = [&](size_t bytes) { char *r = q; q += a256(bytes); return r; };
    uint32_t *status = (uint32_t *)take(256);
    uint64_t *bait_slot = (uint64_t *)take(8 * (size_t)a.nid), *oe_slot = (uint64_t *)take(8 * (size_t)a.nid);
    uint64_t *pair_key = (uint64_t *)take(8 * CHICDIFF_CHICAGO_MAX_PAIRS);
    uint32_t *pair_row = (uint32_t *)take(4 * CHICDIFF_CHICAGO_MAX_PAIRS);
    uint64_t *db_min = (uint64_t *)take(8 * (CHICDIFF_CHICAGO_MAX_DISTBIN + 1)), *db_max = (uint64_t *)take(8 * (CHICDIFF_CHICAGO_MAX_DISTBIN + 1));
    *status_out = status;
    const int32_t npairs = a.ntblb * a.ntlb, ndb = a.ndistbin + 1;
    const unsigned blocks = (unsigned)((a.nrows + CHICDIFF_CHICAGO_ROWS_PER_WORKGROUP - 1) / CHICDIFF_CHICAGO_ROWS_PER_WORKGROUP);
    if (stage == 0) {
        const int64_t ib = ((int64_t)a.nid + 255) / 256;
        chicago_init_kernel<<<(unsigned)(ib < 1 ? 1 : (ib > 2048 ? 2048 : ib)), 256, 0, st>>>(bait_slot, oe_slot, a.nid, pair_key, pair_row, npairs,
                                                                                            db_min, db_max, ndb, status, a.sj, a.si, a.tblb_of,
                                                                                            a.tlb_of);
    } else if (stage == 1) {
        chicago_pass1_kernel<<<blocks, 256, 0, st>>>(a.bait, a.oe, a.tblb, a.tlb, a.distbin, a.refBinMean, a.nrows, a.id_min, a.nid, a.ntblb,
                                                     a.ntlb, a.ndistbin, merge, bait_slot, oe_slot, pair_key, db_min, db_max, status);
    } else {
        chicago_pass2_kernel<<<blocks, 256, 0, st>>>(a.bait, a.oe, a.tblb, a.tlb, a.s_j, a.s_i, a.nrows, a.id_min, a.nid, a.ntblb, a.ntlb, bait_slot,
                                                     oe_slot, pair_key, pair_row, a.sj, a.si, a.tblb_of, a.tlb_of);
        chicago_epilogue_kernel<<<(unsigned)((npairs + ndb + 255) / 256), 256, 0, st>>>(a.Tmean, pair_row, npairs, db_min, db_max, ndb, a.T, a.ref,
                                                                                       status);
    }
}

}  // namespace cd
