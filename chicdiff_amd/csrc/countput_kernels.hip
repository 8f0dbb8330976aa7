// countput_kernels.hip — countput of one condition (chicdiff.R:708-735 the rows kept, :754-768 the aggregation) on the device: the
// pandas groupby of pipeline._countput, bit for bit and in its row order.  The rule is stated above chicdiff_hip_countput_dev in
// include/chicdiff_hip.h.  gfx950 only.
//
//   x[!is.na(distSign)], merge(x, rmap_copy) (:715, :724) -> countput_key_kernel: one row per lane over the concatenated replicates; key
//                                                            = (baitID, otherEndID), all ones = dropped; value = the global row g
//   by = c("baitID", "otherEndID") (:761)                 -> one stable 64-bit radix sort of (key, g): a group's rows lie together in
//                                                            ascending g, and its head is its first appearance
//   order of the groups (groupby(sort = False))           -> countput_heads_kernel marks flag[g of the head]; an exclusive scan of the
//                                                            flags is each group's output row — no second sort
//   mean(N), mean(Bmean), max(score), midpoint[1]         -> countput_reduce_kernel: the head's lane walks its group and runs the
//                                                            sequential rule; a Kahan sum in row order cannot be split across lanes
//
// No value passes through an atomic (the one atomic counts kept rows), and every sum is formed by one lane in the order of g: launch
// shape and arrival order cannot show in a bit.  No kernel here takes a lock or polls.
#include <string.h>

#include <rocprim/rocprim.hpp>

#include "common.h"

namespace cd {

namespace {

constexpr int kCpMaxRep = CHICDIFF_COUNTPUT_MAX_REP;
constexpr int kCpKeyRows = CHICDIFF_COUNTPUT_KEY_ROWS_PER_WORKGROUP;
constexpr int kCpReduceRows = CHICDIFF_COUNTPUT_REDUCE_ROWS_PER_WORKGROUP;
constexpr uint64_t kCpDropped = ~0ull;  // key of a dropped row: behind every kept one (no map ID is INT32_MAX: checked by the caller)
static_assert(kCpKeyRows % 256 == 0 && kCpReduceRows == 256, "the kernels below run 256 lanes per workgroup");
static_assert(sizeof(CountputRep) == 56, "the replicate table is copied as 7 words per entry");

// signed pairs in unsigned radix order, as control_kernels.hip's keys: each half has its sign bit flipped
__device__ __forceinline__ uint64_t cp_key(int32_t bait, int32_t oe) {
    return ((uint64_t)((uint32_t)bait ^ 0x80000000u) << 32) | (uint64_t)((uint32_t)oe ^ 0x80000000u);
}

// the replicate table in LDS (nrep <= 64 entries of 7 words)
__device__ __forceinline__ void cp_load_reps(CountputRep *s_rep, const CountputRep *__restrict__ reps, int nrep) {
    const unsigned long long *src = reinterpret_cast<const unsigned long long *>(reps);
    unsigned long long *dst = reinterpret_cast<unsigned long long *>(s_rep);
    for (int t = threadIdx.x; t < nrep * 7; t += 256) dst[t] = src[t];
    __syncthreads();
}

// the replicate that holds global row g: the LAST one whose first row is <= g (a replicate without rows shares its offset with its
// successor, which is the one that holds the row)
__device__ __forceinline__ int cp_rep_of(const CountputRep *s_rep, int nrep, int64_t g) {
    int lo = 0, hi = nrep;
    while (hi - lo > 1) {
        const int mid = (lo + hi) >> 1;
        if (s_rep[mid].offset <= g) lo = mid; else hi = mid;
    }
    return lo;
}

// ---- keys ------------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void countput_key_kernel(const CountputRep *__restrict__ reps, int nrep, int64_t n, int32_t id_min, int32_t nid,
                                                           const int32_t *__restrict__ chr, uint64_t *__restrict__ keys,
                                                           uint32_t *__restrict__ rows, CountputResult *res) {
    __shared__ CountputRep s_rep[kCpMaxRep];
    __shared__ unsigned int s_kept;
    if (threadIdx.x == 0) s_kept = 0;
    cp_load_reps(s_rep, reps, nrep);
    const int64_t base = (int64_t)blockIdx.x * kCpKeyRows;
    unsigned int kept = 0;
    for (int k = 0; k < kCpKeyRows / 256; k++) {
        const int64_t g = base + k * 256 + threadIdx.x;
        if (g >= n) break;
        const CountputRep &r = s_rep[cp_rep_of(s_rep, nrep, g)];
        const int64_t i = g - r.offset;
        const int32_t bait = r.bait[i], oe = r.oe[i];
        const double ds = r.distSign[i];
        const int64_t rel = (int64_t)oe - (int64_t)id_min;
        bool keep = ds == ds && rel >= 0 && rel < (int64_t)nid;
        if (keep) keep = chr[rel] >= 0;
        keys[g] = keep ? cp_key(bait, oe) : kCpDropped;
        rows[g] = (uint32_t)g;
        kept += keep ? 1u : 0u;
    }
    if (kept) atomicAdd(&s_kept, kept);
    __syncthreads();
    if (threadIdx.x == 0 && s_kept) atomicAdd(&res->nkept, (unsigned long long)s_kept);
}

// ---- heads -----------------------------------------------------------------------------------------------------------------------
// sorted position i is a head when its key is kept and its left neighbour's differs; flag[] was zeroed on the stream
__global__ __launch_bounds__(256) void countput_heads_kernel(const uint64_t *__restrict__ keys, const uint32_t *__restrict__ rows, int64_t n,
                                                             uint32_t *__restrict__ flag) {
    const int64_t i = (int64_t)blockIdx.x * kCpReduceRows + threadIdx.x;
    if (i >= n) return;
    const uint64_t key = keys[i];
    if (key != kCpDropped && (i == 0 || keys[i - 1] != key)) flag[rows[i]] = 1u;
}

// ---- the sequential rule, one group per lane ----------------------------------------------------------------------------------------
struct CpKahan {
    double s = 0.0, c = 0.0, cnt = 0.0;
    __device__ __forceinline__ void add(double v) {
        if (v != v) return;
        cnt += 1.0;
        const double y = v - c;
        const double t = s + y;
        c = (t - s) - y;
        if (c != c) c = 0.0;
        s = t;
    }
    __device__ __forceinline__ double mean() const { return cnt > 0.0 ? s / cnt : __builtin_nan(""); }
};

__global__ __launch_bounds__(256) void countput_reduce_kernel(const CountputRep *__restrict__ reps, int nrep, const uint64_t *__restrict__ keys,
                                                              const uint32_t *__restrict__ rows, int64_t n, const uint32_t *__restrict__ flag,
                                                              const uint32_t *__restrict__ slot, int32_t id_min,
                                                              const int64_t *__restrict__ midsum, int32_t *__restrict__ out_bait,
                                                              int32_t *__restrict__ out_oe, double *__restrict__ Nav, double *__restrict__ Bav,
                                                              double *__restrict__ score, double *__restrict__ mid, CountputResult *res) {
    __shared__ CountputRep s_rep[kCpMaxRep];
    cp_load_reps(s_rep, reps, nrep);
    const int64_t i = (int64_t)blockIdx.x * kCpReduceRows + threadIdx.x;
    if (i == 0) res->ngroups = (unsigned long long)slot[n - 1] + (unsigned long long)flag[n - 1];
    if (i >= n) return;
    const uint64_t key = keys[i];
    if (key == kCpDropped || (i > 0 && keys[i - 1] == key)) return;
    CpKahan sn, sb;
    double best = 0.0;
    bool have = false;
    for (int64_t j = i; j < n && keys[j] == key; j++) {  // the group's rows, ascending g (the sort is stable)
        const int64_t g = rows[j];
        const CountputRep &r = s_rep[cp_rep_of(s_rep, nrep, g)];
        const int64_t k = g - r.offset;
        sn.add((double)r.N[k]);
        sb.add(r.Bmean[k]);
        const double v = r.score[k];
        if (v == v && (!have || v > best)) {
            best = v;
            have = true;
        }
    }
    const int32_t oe = (int32_t)((uint32_t)key ^ 0x80000000u);
    const uint32_t o = slot[rows[i]];
    out_bait[o] = (int32_t)((uint32_t)(key >> 32) ^ 0x80000000u);
    out_oe[o] = oe;
    Nav[o] = sn.mean();
    Bav[o] = sb.mean();
    score[o] = have ? best : __builtin_nan("");
    mid[o] = (double)midsum[(int64_t)oe - (int64_t)id_min] / 2.0;
}

size_t cp_c256(size_t x) { return (x + 255) & ~(size_t)255; }

size_t cp_prim_bytes(int64_t n) {
    size_t a = 0, b = 0;
    uint64_t *k = nullptr;
    uint32_t *v = nullptr;
    (void)rocprim::radix_sort_pairs(nullptr, a, k, k, v, v, (size_t)n, 0, 64, (hipStream_t)0);
    (void)rocprim::exclusive_scan(nullptr, b, v, v, 0u, (size_t)n, rocprim::plus<uint32_t>(), (hipStream_t)0);
    return (a > b ? a : b) + 256;
}

}  // namespace

size_t countput_workspace_bytes(int64_t n) {
    return cp_c256(sizeof(CountputResult)) + cp_c256(sizeof(CountputRep) * kCpMaxRep) + 2 * cp_c256(sizeof(uint64_t) * (size_t)n) +
           2 * cp_c256(sizeof(uint32_t) * (size_t)n) + cp_prim_bytes(n);
}

// Everything is enqueued on `st`; *res_out is where the counts end up (device memory inside ws).
int launch_countput(const CountputArgs &a, char *ws, hipStream_t st, const CountputResult **res_out) {
    const int64_t n = a.n;
    char *q = ws;
    auto take = [&](size_t bytes) { char *r = q; q += cp_c256(bytes); return r; };
    CountputResult *res = (CountputResult *)take(sizeof(CountputResult));
    CountputRep *d_reps = (CountputRep *)take(sizeof(CountputRep) * kCpMaxRep);
    uint64_t *ka = (uint64_t *)take(8 * (size_t)n), *kb = (uint64_t *)take(8 * (size_t)n);
    uint32_t *va = (uint32_t *)take(4 * (size_t)n), *vb = (uint32_t *)take(4 * (size_t)n);
    void *tmp = q;
    size_t tmp_bytes = cp_prim_bytes(n);
    uint32_t *flag = (uint32_t *)ka, *slot = flag + n;  // the unsorted keys are done with once the sort has run: 8 n bytes for two words per row
    *res_out = res;

    if (hipMemsetAsync(res, 0, sizeof(CountputResult), st) != hipSuccess) return 1;
    if (hipMemcpyAsync(d_reps, a.reps, sizeof(CountputRep) * (size_t)a.nrep, hipMemcpyHostToDevice, st) != hipSuccess) return 1;
    countput_key_kernel<<<(unsigned)((n + kCpKeyRows - 1) / kCpKeyRows), 256, 0, st>>>(d_reps, a.nrep, n, a.id_min, a.nid, a.chr, ka, va, res);
    if (rocprim::radix_sort_pairs(tmp, tmp_bytes, ka, kb, va, vb, (size_t)n, 0, 64, st) != hipSuccess) return 1;
    if (hipMemsetAsync(flag, 0, sizeof(uint32_t) * (size_t)n, st) != hipSuccess) return 1;
    const unsigned blocks = (unsigned)((n + kCpReduceRows - 1) / kCpReduceRows);
    countput_heads_kernel<<<blocks, 256, 0, st>>>(kb, vb, n, flag);
    if (rocprim::exclusive_scan(tmp, tmp_bytes, flag, slot, 0u, (size_t)n, rocprim::plus<uint32_t>(), st) != hipSuccess) return 1;
    countput_reduce_kernel<<<blocks, 256, 0, st>>>(d_reps, a.nrep, kb, vb, n, flag, slot, a.id_min, a.midsum, a.out_bait, a.out_oe, a.Nav, a.Bav,
                                                   a.score, a.mid, res);
    return 0;
}

}  // namespace cd
