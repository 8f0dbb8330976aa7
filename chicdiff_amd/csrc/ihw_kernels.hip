// ihw_kernels.hip — training the IHW weights on the device (the rule is above chicdiff_hip_ihw_train_dev in include/chicdiff_hip.h):
// groups, folds, the Grenander estimator of every (fold, group) and the weights of every fold.  gfx950 only.
//
//   kept rows, keys, m         -> ihw_key_kernel: order-preserving 64-bit keys of the covariate and of p; refusals as smallest rows
//   rank, group, fold          -> one stable radix sort of (covariate key, row), ihw_plan_kernel (group edges by bisection of the
//                                 monotone rank -> group rule, chunk bases), ihw_group_kernel
//   one sort for every fold    -> stable sort by p, stable sort by group (9 bits), ihw_gather_kernel: (p, fold) in (group, p) order
//   chunk bases                -> ihw_hist_kernel + one exclusive scan: per (fold, chunk) the rows of that fold before the chunk
//   chunk hulls                -> ihw_hull_kernel: (p, fold) of four chunks in LDS, one lane per (chunk, fold) runs the monotone chain
//   merge                      -> ihw_merge_kernel, once per level: one lane joins kIhwFanIn neighbouring hulls in place
//   segments, order, sweep     -> ihw_segcount_kernel + scan, ihw_segfill_kernel, one radix sort by slope, ihw_seggather_kernel,
//                                 ihw_sweep_kernel (one lane per fold: a running double sum in a fixed order)
//
// The knot test is exact (ihw.h), and hull(A u B) = hull(hull A u hull B): the knots do not depend on chunk length, launch shape or
// arrival order.  Only integers pass through atomics (the kept count, the smallest refused row).
#include <math.h>
#include <string.h>

#include <rocprim/rocprim.hpp>

#include "common.h"
#include "ihw.h"
#include "philox.h"

namespace cd {

namespace {

constexpr uint64_t kDropped = ~0ull;

__device__ __forceinline__ uint64_t order_key(double v) {
    const uint64_t b = (uint64_t)__double_as_longlong(v);
    return (b >> 63) ? ~b : (b | 0x8000000000000000ull);
}

__global__ __launch_bounds__(256) void ihw_key_kernel(const double *__restrict__ pvalue, const double *__restrict__ cov, int64_t n,
                                                      uint64_t *covkey, uint64_t *pkey, uint32_t *iota, IhwDev *dev) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    bool kept = false;
    if (i < n) {
        const double p = pvalue[i];
        uint64_t ck = kDropped, pk = kDropped;
        if (p == p) {
            kept = true;
            if (!(p >= 0.0 && p <= 1.0)) atomicMin(&dev->bad_p, (unsigned long long)i);
            const double cv = cov[i];
            if (cv != cv) atomicMin(&dev->bad_cov, (unsigned long long)i);
            ck = order_key(cv + 0.0);  // -0 + 0 = +0: the two zeros are one key
            pk = (uint64_t)__double_as_longlong(p + 0.0);
        }
        covkey[i] = ck;
        pkey[i] = pk;
        iota[i] = (uint32_t)i;
    }
    const uint64_t kb = __ballot(kept);
    if ((threadIdx.x & 63) == 0 && kb) atomicAdd(&dev->m, (unsigned int)__popcll(kb));
}

// one workgroup: nbins, the verdict, the first rank of every group and the first chunk of every group
__global__ __launch_bounds__(320) void ihw_plan_kernel(IhwDev *dev, int nbins_arg, int L, uint32_t *gs, uint32_t *chunk0) {
    __shared__ uint32_t s_gs[kIhwMaxBins + 1];
    const uint32_t m = dev->m;
    uint32_t nb = nbins_arg > 0 ? (uint32_t)nbins_arg : m / 1500u;
    if (nbins_arg <= 0) nb = nb < 1u ? 1u : (nb > (uint32_t)kIhwAutoMaxBins ? (uint32_t)kIhwAutoMaxBins : nb);
    const bool ok = dev->bad_p == ~0ull && dev->bad_cov == ~0ull && m > 0 && nb <= m;
    const uint32_t t = threadIdx.x;
    if (ok && t <= nb) {  // ranks 1 .. m with group <= t: the rule is monotone in the rank
        uint32_t lo = 0, hi = m;
        while (lo < hi) {
            const uint32_t mid = lo + (hi - lo + 1) / 2;
            if (ihw_group_of_rank(mid, m, nb) <= t) lo = mid; else hi = mid - 1;
        }
        s_gs[t] = lo;
        gs[t] = lo;
    }
    __syncthreads();
    if (t == 0) {
        uint32_t acc = 0;
        if (ok) {
            for (uint32_t g = 0; g < nb; g++) {
                const uint32_t sz = s_gs[g + 1] - s_gs[g], ch = (sz + (uint32_t)L - 1) / (uint32_t)L;
                chunk0[g] = acc;
                acc += ch < 1u ? 1u : ch;  // an empty group keeps one (empty) chunk: its estimator has the two end knots
            }
            chunk0[nb] = acc;
        }
        dev->nbins = nb;
        dev->nchunks = acc;
        dev->ok = ok ? 1u : 0u;
    }
}

__global__ __launch_bounds__(256) void ihw_group_kernel(const uint32_t *__restrict__ rows, int64_t n, const IhwDev *__restrict__ dev,
                                                        int nfolds, uint64_t seed, int32_t *group, int32_t *fold) {
    const int64_t k = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (k >= n) return;
    const uint32_t row = rows[k];
    if (dev->ok && k < (int64_t)dev->m) {
        group[row] = (int32_t)ihw_group_of_rank((uint32_t)k + 1u, dev->m, dev->nbins);
        const Philox4 r = philox4x32_10(row, 0u, 0u, kIhwStream, (uint32_t)seed, (uint32_t)(seed >> 32));
        fold[row] = (int32_t)(((uint64_t)r.w[0] * (uint64_t)nfolds) >> 32);
    } else {
        group[row] = INT32_MIN;
        fold[row] = -1;
    }
}

__global__ __launch_bounds__(256) void ihw_gkey_kernel(const uint32_t *__restrict__ rows, int64_t n, const int32_t *__restrict__ group,
                                                       uint32_t *gkey) {
    const int64_t k = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (k >= n) return;
    const int32_t g = group[rows[k]];
    gkey[k] = g == INT32_MIN ? (uint32_t)kIhwMaxBins : (uint32_t)(g - 1);
}

__global__ __launch_bounds__(256) void ihw_gather_kernel(const uint32_t *__restrict__ rows, int64_t n, const IhwDev *__restrict__ dev,
                                                         const double *__restrict__ pvalue, const int32_t *__restrict__ fold, double *sp,
                                                         uint8_t *sf) {
    const int64_t k = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (k >= n || !dev->ok || k >= (int64_t)dev->m) return;
    const uint32_t row = rows[k];
    sp[k] = pvalue[row] + 0.0;
    sf[k] = (uint8_t)fold[row];
}

// chunk c -> its group (0-based) and its rows [start, end) of the (group, p) order
__device__ __forceinline__ void chunk_span(uint32_t c, const uint32_t *__restrict__ chunk0, const uint32_t *__restrict__ gs, uint32_t nb,
                                           uint32_t L, uint32_t &g, uint32_t &start, uint32_t &end) {
    uint32_t lo = 0, hi = nb - 1;  // the last group with chunk0[g] <= c
    while (lo < hi) {
        const uint32_t mid = (lo + hi + 1) >> 1;
        if (chunk0[mid] <= c) lo = mid; else hi = mid - 1;
    }
    g = lo;
    const uint32_t g1 = gs[g + 1];
    const uint64_t s = (uint64_t)gs[g] + (uint64_t)(c - chunk0[g]) * L;
    start = s > g1 ? g1 : (uint32_t)s;
    end = s + L > g1 ? g1 : (uint32_t)(s + L);
}

// hist[f * (CC + 1) + c] = rows of fold f in chunk c (0 behind the last chunk)
__global__ __launch_bounds__(256) void ihw_hist_kernel(const IhwDev *__restrict__ dev, const uint32_t *__restrict__ chunk0,
                                                       const uint32_t *__restrict__ gs, const uint8_t *__restrict__ sf, int nfolds, int64_t CC,
                                                       int L, uint32_t *hist) {
    const int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (idx >= (int64_t)nfolds * (CC + 1)) return;
    const uint32_t f = (uint32_t)(idx / (CC + 1)), c = (uint32_t)(idx % (CC + 1));
    uint32_t v = 0;
    if (c < dev->nchunks) {
        uint32_t g, start, end;
        chunk_span(c, chunk0, gs, dev->nbins, (uint32_t)L, g, start, end);
        for (uint32_t k = start; k < end; k++) v += sf[k] == f;
    }
    hist[idx] = v;
}

// ---- chunk hulls ------------------------------------------------------------------------------------------------------------------
// A workgroup of one wave takes four chunks: their (p, fold) go to LDS, lane (chunk, f) runs the monotone chain over the chunk's rows
// whose fold is not f.  A stack word is (index in the chunk | rows taken so far << 8); index 128 / 129 = the end points (0, 0) and
// (1, M), which the first and the last chunk of a group add.  The survivors go to the chunk's L + 2 slots of fold f.
constexpr uint32_t kAnchor0 = 128, kAnchor1 = 129;

__global__ __launch_bounds__(64) void ihw_hull_kernel(const IhwDev *__restrict__ dev, const uint32_t *__restrict__ chunk0,
                                                      const uint32_t *__restrict__ gs, const double *__restrict__ sp,
                                                      const uint8_t *__restrict__ sf, const uint32_t *__restrict__ S, int nfolds, int64_t CC,
                                                      int64_t SL, int L, double *hx, uint32_t *hc, uint32_t *cnt) {
    __shared__ double s_p[4][kIhwMaxChunk];
    __shared__ uint8_t s_f[4][kIhwMaxChunk];
    __shared__ uint32_t s_stk[kIhwMaxChunk + 2][64];
    __shared__ uint32_t s_g[4], s_start[4], s_end[4];
    const uint32_t lane = threadIdx.x, nchunks = dev->nchunks, nb = dev->nbins;
    if (lane < 4) {
        const uint32_t c = blockIdx.x * 4 + lane;
        uint32_t g = 0, start = 0, end = 0;
        if (c < nchunks) chunk_span(c, chunk0, gs, nb, (uint32_t)L, g, start, end);
        s_g[lane] = g;
        s_start[lane] = start;
        s_end[lane] = end;
    }
    __syncthreads();
    for (int ci = 0; ci < 4; ci++) {
        const uint32_t start = s_start[ci], len = s_end[ci] - start;
        for (uint32_t j = lane; j < len; j += 64) {
            s_p[ci][j] = sp[start + j];
            s_f[ci][j] = sf[start + j];
        }
    }
    __syncthreads();
    const uint32_t ci = lane >> 4, f = lane & 15, c = blockIdx.x * 4 + ci;
    if (c >= nchunks || f >= (uint32_t)nfolds) return;
    const uint32_t g = s_g[ci], start = s_start[ci], len = s_end[ci] - start;
    const uint32_t *Sf = S + (int64_t)f * (CC + 1);
    const uint32_t c_first = chunk0[g], c_end = chunk0[g + 1];
    const uint32_t M = (gs[g + 1] - gs[g]) - (Sf[c_end] - Sf[c_first]);      // rows of the group outside fold f
    const uint32_t base = (start - gs[g]) - (Sf[c] - Sf[c_first]);            // ... of them before this chunk
    const double *P = s_p[ci];
    auto X = [&](uint32_t e) { const uint32_t j = e & 255u; return j == kAnchor0 ? 0.0 : j == kAnchor1 ? 1.0 : P[j]; };
    auto C = [&](uint32_t e) { return base + (e >> 8); };
    uint32_t sz = 0;
    auto push = [&](uint32_t e) {
        const double qx = X(e);
        const uint32_t qc = C(e);
        while (sz > 0 && X(s_stk[sz - 1][lane]) == qx) sz--;  // equal x: only the larger count is a point
        while (sz >= 2) {
            const uint32_t a = s_stk[sz - 2][lane], b = s_stk[sz - 1][lane];
            if (ihw_orient(X(a), C(a), X(b), C(b), qx, qc) > 0) break;
            sz--;
        }
        s_stk[sz++][lane] = e;
    };
    uint32_t taken = 0;
    if (c == c_first) push(kAnchor0);
    for (uint32_t j = 0; j < len; j++)
        if (s_f[ci][j] != f) push(j | (++taken << 8));
    if (c + 1 == c_end) {
        if (M == 0) taken = 1;  // an empty training set: the knots (0, 0), (1, 1), M taken as 1 (base is 0)
        push(kAnchor1 | (taken << 8));
    }
    const int64_t slot = (int64_t)f * SL + (int64_t)c * (L + 2);
    for (uint32_t j = 0; j < sz; j++) {
        const uint32_t e = s_stk[j][lane];
        hx[slot + j] = X(e);
        hc[slot + j] = C(e);
    }
    cnt[(int64_t)f * CC + c] = sz;
}

// One level of the merge: the node of chunk c (the first of stride * kIhwFanIn chunks of its group) joins the hulls of its children,
// which start `stride` chunks apart, in place: the stack grows from the node's first slot and never passes the slot being read.
__global__ __launch_bounds__(256) void ihw_merge_kernel(const IhwDev *__restrict__ dev, const uint32_t *__restrict__ chunk0,
                                                        const uint32_t *__restrict__ gs, int nfolds, int64_t CC, int64_t SL, int L,
                                                        uint32_t stride, double *hx, uint32_t *hc, uint32_t *cnt) {
    const int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (idx >= (int64_t)nfolds * CC) return;
    const uint32_t f = (uint32_t)(idx / CC), c = (uint32_t)(idx % CC);
    if (c >= dev->nchunks) return;
    uint32_t g, start, end;
    chunk_span(c, chunk0, gs, dev->nbins, (uint32_t)L, g, start, end);
    const uint64_t q = c - chunk0[g];
    if (q % ((uint64_t)stride * kIhwFanIn) != 0) return;
    const uint32_t c_end = chunk0[g + 1];
    double *X = hx + (int64_t)f * SL;
    uint32_t *Cn = hc + (int64_t)f * SL, *K = cnt + (int64_t)f * CC;
    const int64_t out = (int64_t)c * (L + 2);
    uint32_t sz = K[c];
    for (int i = 1; i < kIhwFanIn; i++) {
        const uint64_t cc = (uint64_t)c + (uint64_t)i * stride;
        if (cc >= c_end) break;
        const uint32_t k = K[cc];
        const int64_t in = (int64_t)cc * (L + 2);
        for (uint32_t j = 0; j < k; j++) {
            const double qx = X[in + j];
            const uint32_t qc = Cn[in + j];
            while (sz > 0 && X[out + sz - 1] == qx) sz--;
            while (sz >= 2) {
                if (ihw_orient(X[out + sz - 2], Cn[out + sz - 2], X[out + sz - 1], Cn[out + sz - 1], qx, qc) > 0) break;
                sz--;
            }
            X[out + sz] = qx;
            Cn[out + sz] = qc;
            sz++;
        }
    }
    K[c] = sz;
}

// ---- segments ---------------------------------------------------------------------------------------------------------------------
// nseg[f * NB + g] = knots - 1 of (f, g); 0 behind the groups in use and in the one entry behind the table
__global__ __launch_bounds__(256) void ihw_segcount_kernel(const IhwDev *__restrict__ dev, const uint32_t *__restrict__ chunk0,
                                                           const uint32_t *__restrict__ cnt, int nfolds, int NB, int64_t CC, uint32_t *nseg) {
    const int idx = blockIdx.x * 256 + threadIdx.x;
    if (idx > nfolds * NB) return;
    uint32_t v = 0;
    const uint32_t f = (uint32_t)(idx / NB), g = (uint32_t)(idx % NB);
    if (idx < nfolds * NB && dev->ok && g < dev->nbins) v = cnt[(int64_t)f * CC + chunk0[g]] - 1u;
    nseg[idx] = v;
}

__global__ __launch_bounds__(256) void ihw_segfill_kernel(const uint32_t *__restrict__ chunk0, const uint32_t *__restrict__ segoff,
                                                          const uint32_t *__restrict__ nseg, const double *__restrict__ hx,
                                                          const uint32_t *__restrict__ hc, int nfolds, int NB, int64_t SL, int L, int64_t total,
                                                          uint64_t *key, uint32_t *val, uint32_t *gf, double *sd, double *sdF) {
    const int64_t off = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (off >= total) return;
    uint32_t lo = 0, hi = (uint32_t)(nfolds * NB - 1);  // the last entry with segoff[e] <= off
    while (lo < hi) {
        const uint32_t mid = (lo + hi + 1) >> 1;
        if ((int64_t)segoff[mid] <= off) lo = mid; else hi = mid - 1;
    }
    const uint32_t f = lo / (uint32_t)NB, g = lo % (uint32_t)NB, j = (uint32_t)(off - segoff[lo]) + 1u, K = nseg[lo] + 1u;
    const int64_t slot = (int64_t)f * SL + (int64_t)chunk0[g] * (L + 2);
    const double M = (double)hc[slot + K - 1];
    const double d = hx[slot + j] - hx[slot + j - 1];
    const double dF = (double)(hc[slot + j] - hc[slot + j - 1]) / M;
    const double s = dF / d;
    key[off] = ~(uint64_t)__double_as_longlong(s);  // s >= +0: descending by slope; ties keep (g, j) order (the sort is stable)
    val[off] = (uint32_t)off;
    gf[off] = g | (f << 16);
    sd[off] = d;
    sdF[off] = dF;
}

__global__ __launch_bounds__(256) void ihw_seggather_kernel(const uint32_t *__restrict__ val, int64_t total, const uint32_t *__restrict__ gf,
                                                            const double *__restrict__ sd, const double *__restrict__ sdF, uint32_t *rgf,
                                                            double *rd, double *rdF) {
    const int64_t k = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (k >= total) return;
    const uint32_t off = val[k];
    rgf[k] = gf[off];
    rd[k] = sd[off];
    rdF[k] = sdF[off];
}

// one lane per fold: step 5 of the rule, every double operation in the stated order
__global__ __launch_bounds__(64) void ihw_sweep_kernel(const uint32_t *__restrict__ chunk0, const uint32_t *__restrict__ S,
                                                       const uint32_t *__restrict__ cnt, const double *__restrict__ hx,
                                                       const uint32_t *__restrict__ hc, const uint32_t *__restrict__ segoff, int nfolds, int nbins,
                                                       int NB, int64_t CC, int64_t SL, int L, int64_t total, double alpha,
                                                       const uint32_t *__restrict__ rgf, const double *__restrict__ rd,
                                                       const double *__restrict__ rdF, uint32_t *hh, double *t, double *w, double *TH,
                                                       uint32_t *nsegf) {
    const uint32_t f = threadIdx.x;
    if (f >= (uint32_t)nfolds) return;
    const uint32_t *Sf = S + (int64_t)f * (CC + 1);
    uint32_t *h = hh + (int64_t)f * NB;
    double *tg = t + (int64_t)f * NB;
    uint64_t H = 0;
    double B = 0.0;
    for (int g = 0; g < nbins; g++) {
        const uint32_t hg = Sf[chunk0[g + 1]] - Sf[chunk0[g]];
        const int64_t slot = (int64_t)f * SL + (int64_t)chunk0[g] * (L + 2);
        const uint32_t K = cnt[(int64_t)f * CC + chunk0[g]];
        const double F0 = (double)hc[slot] / (double)hc[slot + K - 1];
        B = B - (alpha * (double)hg) * F0;
        H += hg;
        h[g] = hg;
        tg[g] = 0.0;
    }
    for (int64_t k = 0; k < total; k++) {
        const uint32_t e = rgf[k];
        if ((e >> 16) != f) continue;
        const uint32_t g = e & 0xffffu;
        const double d = rd[k], dF = rdF[k];
        const double cost = (double)h[g] * (d - alpha * dF);
        if (B + cost <= 0.0) {
            tg[g] = tg[g] + d;
            B = B + cost;
        } else {
            tg[g] = tg[g] + (-B / cost) * d;
            break;
        }
    }
    double T = 0.0;
    for (int g = 0; g < nbins; g++) T = T + (double)h[g] * tg[g];
    for (int g = 0; g < nbins; g++) w[g + (int64_t)nbins * f] = T == 0.0 ? 1.0 : (tg[g] * (double)H) / T;
    TH[2 * f] = T;
    TH[2 * f + 1] = (double)H;
    nsegf[f] = segoff[(f + 1) * NB] - segoff[f * NB];
}

__global__ __launch_bounds__(256) void ihw_knots_out_kernel(const uint32_t *__restrict__ chunk0, const uint32_t *__restrict__ segoff,
                                                            const uint32_t *__restrict__ nseg, const double *__restrict__ hx,
                                                            const uint32_t *__restrict__ hc, int nfolds, int nbins, int NB, int64_t SL, int L,
                                                            int64_t *ptr, double *x, int32_t *cc) {
    const int q = blockIdx.x * 256 + threadIdx.x;
    if (q >= nfolds * nbins) return;
    const int f = q / nbins, g = q % nbins, e = f * NB + g;
    const int64_t off = (int64_t)segoff[e] + q, slot = (int64_t)f * SL + (int64_t)chunk0[g] * (L + 2);
    const uint32_t K = nseg[e] + 1u;
    ptr[q] = off;
    if (q == nfolds * nbins - 1) ptr[q + 1] = off + K;
    for (uint32_t j = 0; j < K; j++) {
        x[off + j] = hx[slot + j];
        cc[off + j] = (int32_t)hc[slot + j];
    }
}

size_t c256(size_t x) { return (x + 255) & ~(size_t)255; }

size_t prim_bytes(const IhwDims &d) {
    size_t best = 0, t = 0;
    uint64_t *k = nullptr;
    uint32_t *v = nullptr;
    (void)rocprim::radix_sort_pairs(nullptr, t, k, k, v, v, (size_t)d.n, 0, 64, (hipStream_t)0);
    best = t;
    (void)rocprim::radix_sort_pairs(nullptr, t, v, v, v, v, (size_t)d.n, 0, 9, (hipStream_t)0);
    best = t > best ? t : best;
    (void)rocprim::exclusive_scan(nullptr, t, v, v, 0u, (size_t)d.nfolds * (size_t)(d.CC + 1), rocprim::plus<uint32_t>(), (hipStream_t)0);
    best = t > best ? t : best;
    (void)rocprim::exclusive_scan(nullptr, t, v, v, 0u, (size_t)d.nfolds * (size_t)d.nb_cap + 1, rocprim::plus<uint32_t>(), (hipStream_t)0);
    best = t > best ? t : best;
    return best + 256;
}

template <class F>
size_t walk_work(const IhwDims &d, F take) {
    const size_t n = (size_t)d.n, F_ = (size_t)d.nfolds, CC = (size_t)d.CC, SL = (size_t)d.SL, NBT = F_ * (size_t)d.nb_cap + 1;
    size_t total = 0;
    total += take(0, sizeof(IhwDev));
    for (int i = 1; i <= 3; i++) total += take(i, 8 * n);
    for (int i = 4; i <= 9; i++) total += take(i, 4 * n);
    total += take(10, 8 * n);                      // sp
    total += take(11, n);                          // sf
    total += take(12, 4 * (size_t)(d.nb_cap + 2));  // gs
    total += take(13, 4 * (size_t)(d.nb_cap + 2));  // chunk0
    total += take(14, 4 * F_ * (CC + 1));          // hist
    total += take(15, 4 * F_ * (CC + 1));          // S
    total += take(16, 4 * F_ * CC);                // cnt
    total += take(17, 4 * F_ * SL);                // hc
    total += take(18, 4 * NBT);                    // nseg
    total += take(19, 4 * NBT);                    // segoff
    total += take(20, 8 * F_ * SL);                // hx
    total += take(21, 4 * n);                      // fold (when the caller wants none)
    total += take(22, prim_bytes(d));
    return total;
}

}  // namespace

size_t ihw_work_bytes(const IhwDims &d) {
    return walk_work(d, [](int, size_t b) { return c256(b); });
}

void ihw_carve(const IhwDims &d, char *ws, IhwWork &w) {
    char *q = ws;
    void *p[23];
    size_t last = 0;
    walk_work(d, [&](int i, size_t b) { p[i] = q; q += c256(b); last = b; return c256(b); });
    w.dev = (IhwDev *)p[0];
    w.k0 = (uint64_t *)p[1]; w.k1 = (uint64_t *)p[2]; w.k2 = (uint64_t *)p[3];
    w.r0 = (uint32_t *)p[4]; w.r1 = (uint32_t *)p[5]; w.r2 = (uint32_t *)p[6]; w.r3 = (uint32_t *)p[7];
    w.g0 = (uint32_t *)p[8]; w.g1 = (uint32_t *)p[9];
    w.sp = (double *)p[10]; w.sf = (uint8_t *)p[11];
    w.gs = (uint32_t *)p[12]; w.chunk0 = (uint32_t *)p[13]; w.hist = (uint32_t *)p[14]; w.S = (uint32_t *)p[15];
    w.cnt = (uint32_t *)p[16]; w.hc = (uint32_t *)p[17]; w.nseg = (uint32_t *)p[18]; w.segoff = (uint32_t *)p[19];
    w.hx = (double *)p[20]; w.fold_tmp = (int32_t *)p[21];
    w.tmp = p[22];
    w.tmp_bytes = last;
}

namespace {
template <class F>
size_t walk_seg(const IhwDims &d, int64_t total, F take) {
    const size_t t = (size_t)(total > 0 ? total : 1), FN = (size_t)d.nfolds * (size_t)d.nb_cap;
    size_t sum = 0, tb = 0;
    uint64_t *k = nullptr;
    uint32_t *v = nullptr;
    (void)rocprim::radix_sort_pairs(nullptr, tb, k, k, v, v, t, 0, 64, (hipStream_t)0);
    sum += take(0, 8 * t);  // key0
    sum += take(1, 8 * t);  // key1
    sum += take(2, 4 * t);  // val0
    sum += take(3, 4 * t);  // val1
    sum += take(4, 4 * t);  // gf
    sum += take(5, 4 * t);  // rgf
    sum += take(6, 8 * t);  // d
    sum += take(7, 8 * t);  // dF
    sum += take(8, 8 * t);  // rd
    sum += take(9, 8 * t);  // rdF
    sum += take(10, 4 * FN);  // hh
    sum += take(11, 8 * FN);  // t
    sum += take(12, 8 * FN);  // w
    sum += take(13, 8 * 2 * (size_t)d.nfolds);  // T, H
    sum += take(14, 4 * (size_t)d.nfolds);      // segments per fold
    sum += take(15, tb + 256);
    return sum;
}
}  // namespace

size_t ihw_seg_bytes(const IhwDims &d, int64_t total) {
    return walk_seg(d, total, [](int, size_t b) { return c256(b); });
}

void ihw_seg_carve(const IhwDims &d, int64_t total, char *ws, IhwSeg &s) {
    char *q = ws;
    void *p[16];
    size_t last = 0;
    walk_seg(d, total, [&](int i, size_t b) { p[i] = q; q += c256(b); last = b; return c256(b); });
    s.key0 = (uint64_t *)p[0]; s.key1 = (uint64_t *)p[1];
    s.val0 = (uint32_t *)p[2]; s.val1 = (uint32_t *)p[3]; s.gf = (uint32_t *)p[4]; s.rgf = (uint32_t *)p[5];
    s.d = (double *)p[6]; s.dF = (double *)p[7]; s.rd = (double *)p[8]; s.rdF = (double *)p[9];
    s.hh = (uint32_t *)p[10]; s.t = (double *)p[11]; s.w = (double *)p[12]; s.TH = (double *)p[13]; s.nsegf = (uint32_t *)p[14];
    s.tmp = p[15];
    s.tmp_bytes = last;
}

static unsigned blocks_of(int64_t n) { return (unsigned)((n + 255) / 256); }

// keys, the covariate sort, the plan, group and fold at [row]
int launch_ihw_rank(const double *pvalue, const double *cov, const IhwDims &d, int nbins_arg, uint64_t seed, int32_t *group, int32_t *fold,
                    const IhwWork &w, hipStream_t st) {
    IhwDev init;
    memset(&init, 0, sizeof init);
    init.bad_p = init.bad_cov = ~0ull;
    if (hipMemcpyAsync(w.dev, &init, sizeof init, hipMemcpyHostToDevice, st) != hipSuccess) return 1;
    ihw_key_kernel<<<blocks_of(d.n), 256, 0, st>>>(pvalue, cov, d.n, w.k0, w.k2, w.r0, w.dev);
    size_t tb = w.tmp_bytes;
    if (rocprim::radix_sort_pairs(w.tmp, tb, w.k0, w.k1, w.r0, w.r1, (size_t)d.n, 0, 64, st) != hipSuccess) return 1;
    ihw_plan_kernel<<<1, 320, 0, st>>>(w.dev, nbins_arg, d.L, w.gs, w.chunk0);
    ihw_group_kernel<<<blocks_of(d.n), 256, 0, st>>>(w.r1, d.n, w.dev, d.nfolds, seed, group, fold);
    return 0;
}

// the kept rows stably by p, then stably by group: (p, fold) of every row in (group, p, row) order
int launch_ihw_sorts(const double *pvalue, const int32_t *group, const int32_t *fold, const IhwDims &d, const IhwWork &w, hipStream_t st) {
    size_t tb = w.tmp_bytes;
    if (rocprim::radix_sort_pairs(w.tmp, tb, w.k2, w.k0, w.r0, w.r2, (size_t)d.n, 0, 64, st) != hipSuccess) return 1;
    ihw_gkey_kernel<<<blocks_of(d.n), 256, 0, st>>>(w.r2, d.n, group, w.g0);
    tb = w.tmp_bytes;
    if (rocprim::radix_sort_pairs(w.tmp, tb, w.g0, w.g1, w.r2, w.r3, (size_t)d.n, 0, 9, st) != hipSuccess) return 1;
    ihw_gather_kernel<<<blocks_of(d.n), 256, 0, st>>>(w.r3, d.n, w.dev, pvalue, fold, w.sp, w.sf);
    return 0;
}

int launch_ihw_hulls(const IhwDims &d, const IhwWork &w, hipStream_t st) {
    const int64_t nh = (int64_t)d.nfolds * (d.CC + 1);
    ihw_hist_kernel<<<blocks_of(nh), 256, 0, st>>>(w.dev, w.chunk0, w.gs, w.sf, d.nfolds, d.CC, d.L, w.hist);
    size_t tb = w.tmp_bytes;
    if (rocprim::exclusive_scan(w.tmp, tb, w.hist, w.S, 0u, (size_t)nh, rocprim::plus<uint32_t>(), st) != hipSuccess) return 1;
    ihw_hull_kernel<<<(unsigned)((d.CC + 3) / 4), 64, 0, st>>>(w.dev, w.chunk0, w.gs, w.sp, w.sf, w.S, d.nfolds, d.CC, d.SL, d.L, w.hx, w.hc,
                                                              w.cnt);
    return 0;
}

// levels until one node spans the longest group there can be, then the segment counts and their offsets
int launch_ihw_merge(const IhwDims &d, const IhwWork &w, hipStream_t st) {
    for (uint64_t stride = 1; stride * (uint64_t)d.L < (uint64_t)d.n; stride *= kIhwFanIn)
        ihw_merge_kernel<<<blocks_of((int64_t)d.nfolds * d.CC), 256, 0, st>>>(w.dev, w.chunk0, w.gs, d.nfolds, d.CC, d.SL, d.L, (uint32_t)stride,
                                                                              w.hx, w.hc, w.cnt);
    const int ne = d.nfolds * d.nb_cap + 1;
    ihw_segcount_kernel<<<blocks_of(ne), 256, 0, st>>>(w.dev, w.chunk0, w.cnt, d.nfolds, d.nb_cap, d.CC, w.nseg);
    size_t tb = w.tmp_bytes;
    if (rocprim::exclusive_scan(w.tmp, tb, w.nseg, w.segoff, 0u, (size_t)ne, rocprim::plus<uint32_t>(), st) != hipSuccess) return 1;
    return 0;
}

int launch_ihw_sweep(const IhwDims &d, const IhwWork &w, const IhwSeg &s, int64_t total, int nbins, double alpha, hipStream_t st) {
    if (total > 0) {
        ihw_segfill_kernel<<<blocks_of(total), 256, 0, st>>>(w.chunk0, w.segoff, w.nseg, w.hx, w.hc, d.nfolds, d.nb_cap, d.SL, d.L, total, s.key0,
                                                            s.val0, s.gf, s.d, s.dF);
        size_t tb = s.tmp_bytes;
        if (rocprim::radix_sort_pairs(s.tmp, tb, s.key0, s.key1, s.val0, s.val1, (size_t)total, 0, 64, st) != hipSuccess) return 1;
        ihw_seggather_kernel<<<blocks_of(total), 256, 0, st>>>(s.val1, total, s.gf, s.d, s.dF, s.rgf, s.rd, s.rdF);
    }
    ihw_sweep_kernel<<<1, 64, 0, st>>>(w.chunk0, w.S, w.cnt, w.hx, w.hc, w.segoff, d.nfolds, nbins, d.nb_cap, d.CC, d.SL, d.L, total, alpha, s.rgf,
                                       s.rd, s.rdF, s.hh, s.t, s.w, s.TH, s.nsegf);
    return 0;
}

void launch_ihw_knots_out(const IhwDims &d, const IhwWork &w, int nbins, int64_t *ptr, double *x, int32_t *c, hipStream_t st) {
    ihw_knots_out_kernel<<<blocks_of((int64_t)d.nfolds * nbins), 256, 0, st>>>(w.chunk0, w.segoff, w.nseg, w.hx, w.hc, d.nfolds, nbins, d.nb_cap,
                                                                              d.SL, d.L, ptr, x, c);
}

}  // namespace cd
