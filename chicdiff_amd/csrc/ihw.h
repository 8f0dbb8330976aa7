// ihw.h — what the host shares with ihw_kernels.hip: the limits, the device's info block and the exact knot test of the Grenander
// estimator (the rule is above chicdiff_hip_ihw_train_dev in include/chicdiff_hip.h).
#pragma once
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "../../include/chicdiff_hip.h"

namespace cd {

constexpr int kIhwMaxBins = CHICDIFF_IHW_MAX_BINS, kIhwMaxFolds = CHICDIFF_IHW_MAX_FOLDS, kIhwAutoMaxBins = 40;
constexpr int kIhwMaxChunk = 128;  // the longest chunk: one lane's stack of (index, count) words in LDS
constexpr int kIhwFanIn = 16;      // hulls one lane merges per level
constexpr uint32_t kIhwStream = CHICDIFF_IHW_PHILOX_STREAM;
constexpr int kIhwChunkLens[3] = {4, 32, 128};

// the refusals and sizes only the device knows before the first host stop
struct IhwDev {
    unsigned long long bad_p, bad_cov;  // smallest offending row (~0: none)
    uint32_t m, nbins, nchunks, ok;
};

struct IhwDims {  // host-known sizes of one call
    int64_t n;
    int nfolds, nb_cap, L;
    int64_t CC;  // capacity in chunks: ceil(n / L) + nb_cap
    int64_t SL;  // knot slots per fold: CC * (L + 2)
};

struct IhwWork {  // device arrays of one call (carved from the context's scratch)
    IhwDev *dev;
    uint64_t *k0, *k1, *k2;
    uint32_t *r0, *r1, *r2, *r3, *g0, *g1;
    double *sp;
    uint8_t *sf;
    uint32_t *gs, *chunk0, *hist, *S, *cnt, *hc, *nseg, *segoff;
    double *hx;
    int32_t *fold_tmp;
    void *tmp;
    size_t tmp_bytes;
};

struct IhwSeg {  // segment stage (sized by the segment total of the first host stop)
    uint64_t *key0, *key1;
    uint32_t *val0, *val1, *gf, *rgf, *hh;
    double *d, *dF, *rd, *rdF, *t, *w, *TH;
    uint32_t *nsegf;
    void *tmp;
    size_t tmp_bytes;
};

size_t ihw_work_bytes(const IhwDims &d);
void ihw_carve(const IhwDims &d, char *ws, IhwWork &w);
size_t ihw_seg_bytes(const IhwDims &d, int64_t total);
void ihw_seg_carve(const IhwDims &d, int64_t total, char *ws, IhwSeg &s);
int launch_ihw_rank(const double *pvalue, const double *cov, const IhwDims &d, int nbins_arg, uint64_t seed, int32_t *group, int32_t *fold,
                    const IhwWork &w, hipStream_t st);
int launch_ihw_sorts(const double *pvalue, const int32_t *group, const int32_t *fold, const IhwDims &d, const IhwWork &w, hipStream_t st);
int launch_ihw_hulls(const IhwDims &d, const IhwWork &w, hipStream_t st);
int launch_ihw_merge(const IhwDims &d, const IhwWork &w, hipStream_t st);
int launch_ihw_sweep(const IhwDims &d, const IhwWork &w, const IhwSeg &s, int64_t total, int nbins, double alpha, hipStream_t st);
void launch_ihw_knots_out(const IhwDims &d, const IhwWork &w, int nbins, int64_t *ptr, double *x, int32_t *c, hipStream_t st);

// ---- the exact knot test ----------------------------------------------------------------------------------------------------------
__host__ __device__ inline void ihw_two_sum(double a, double b, double &s, double &e) {
    s = a + b;
    const double bb = s - a;
    e = (a - (s - bb)) + (b - bb);
}
__host__ __device__ inline void ihw_two_diff(double a, double b, double &s, double &e) {
    s = a - b;
    const double bv = a - s, av = s + bv;
    e = (a - av) + (bv - b);
}
// sign of (b.c - a.c) * (c.x - a.x) - (c.c - a.c) * (b.x - a.x) in exact arithmetic: +1, 0 or -1.  b is a knot between a and c iff +1.
// x: any doubles of [0, 1] (subnormals included); counts: below 2^31.  First an fp64 evaluation with an error bound; where that does
// not decide, the differences of the x's as two-term expansions, their products with the count differences through fma (every product
// and residue is a multiple of 2^-1074 and representable), and the eight terms summed as a non-overlapping expansion (Shewchuk 1997,
// Grow-Expansion), whose sign is that of its largest non-zero component.
__host__ __device__ inline int ihw_orient(double ax, uint32_t ac, double bx, uint32_t bc, double cx, uint32_t cc) {
    const double n1 = (double)((int64_t)bc - (int64_t)ac), n2 = (double)((int64_t)cc - (int64_t)ac);
    {
        const double p1 = n1 * (cx - ax), p2 = n2 * (bx - ax), det = p1 - p2, mag = fabs(p1) + fabs(p2);
        // three roundings per product and one of the difference: |error| <= 4 * 2^-53 * mag once nothing underflowed
        if (mag > 1e-280 && fabs(det) > 1e-15 * mag) return det > 0.0 ? 1 : -1;
    }
    double h1, l1, h2, l2;
    ihw_two_diff(cx, ax, h1, l1);
    ihw_two_diff(bx, ax, h2, l2);
    const double m2 = -n2;
    double term[8];
    term[0] = n1 * l1;
    term[1] = fma(n1, l1, -term[0]);
    term[2] = m2 * l2;
    term[3] = fma(m2, l2, -term[2]);
    term[4] = n1 * h1;
    term[5] = fma(n1, h1, -term[4]);
    term[6] = m2 * h2;
    term[7] = fma(m2, h2, -term[6]);
    double e[8];
#pragma unroll
    for (int k = 0; k < 8; k++) {
        double q = term[k];
#pragma unroll
        for (int i = 0; i < k; i++) {
            double s, r;
            ihw_two_sum(q, e[i], s, r);
            e[i] = r;
            q = s;
        }
        e[k] = q;
    }
    int sign = 0;
#pragma unroll
    for (int k = 0; k < 8; k++)
        if (e[k] != 0.0) sign = e[k] > 0.0 ? 1 : -1;
    return sign;
}

// group of rank r (1-based) among m kept rows: exactly these two double operations, then the ceiling
__host__ __device__ inline uint32_t ihw_group_of_rank(uint32_t r, uint32_t m, uint32_t nbins) {
    return (uint32_t)ceil(((double)r / (double)m) * (double)nbins);
}

}  // namespace cd
