// ihw_api.hip — entry points of the IHW training stage (ihw_kernels.hip; the rule is in include/chicdiff_hip.h).
#include "ctx.h"
#include "ihw.h"

namespace {

bool chunk_len_ok(int L) {
    for (int v : kIhwChunkLens)
        if (v == L) return true;
    return false;
}

struct IhwRun {
    IhwDims d;
    IhwWork w;
    IhwDev h;
    int64_t total = 0;  // segments of all folds
};

// Everything up to the first host stop: groups and folds at [row], the knots of every (fold, group) in the workspace, the segment
// offsets.  Returns with the stream synchronised and the refusals of the device turned into messages.
int ihw_knots(chicdiff_hip_ctx *c, const char *who, const double *d_pvalue, const double *d_cov, int64_t n, int32_t nbins, int32_t nfolds,
              uint64_t seed, int32_t chunk_len, int32_t *d_group, int32_t *d_fold, IhwRun &r) {
    if (!d_pvalue || !d_cov || !d_group) return fail(c, CHICDIFF_E_INVALID, "%s: bad arguments (a NULL pointer)", who);
    if (nfolds < 2 || nfolds > kIhwMaxFolds) return fail(c, CHICDIFF_E_INVALID, "%s: nfolds = %d (2 <= nfolds <= %d)", who, (int)nfolds, kIhwMaxFolds);
    if (nbins < 0 || nbins > kIhwMaxBins)
        return fail(c, CHICDIFF_E_INVALID, "%s: nbins = %d (0 = auto, else 1 <= nbins <= %d: the limit of ihw_apply)", who, (int)nbins, kIhwMaxBins);
    if (n < 1 || n * (int64_t)nfolds >= (1ll << 31))
        return fail(c, CHICDIFF_E_INVALID, "%s: n = %lld rows (1 <= n and n * nfolds < 2^31)", who, (long long)n);
    if (chunk_len == 0) chunk_len = kIhwMaxChunk;
    if (!chunk_len_ok(chunk_len))
        return fail(c, CHICDIFF_E_INVALID, "%s: chunk length %d is not one of chicdiff_hip_ihw_caps' list", who, (int)chunk_len);
    HIPCHK(c, hipSetDevice(c->device));
    IhwDims &d = r.d;
    d.n = n;
    d.nfolds = nfolds;
    d.nb_cap = nbins > 0 ? nbins : kIhwAutoMaxBins;
    d.L = chunk_len;
    d.CC = (n + d.L - 1) / d.L + d.nb_cap;
    d.SL = d.CC * (d.L + 2);
    if (int rc = ensure_aux(c, ihw_work_bytes(d))) return rc;
    ihw_carve(d, c->aux, r.w);
    int32_t *fold = d_fold ? d_fold : r.w.fold_tmp;
    {
        Scope t(c, "ihw_rank");
        if (launch_ihw_rank(d_pvalue, d_cov, d, nbins, seed, d_group, fold, r.w, c->stream)) return fail(c, CHICDIFF_E_HIP, "%s: copy/sort failed", who);
    }
    {
        Scope t(c, "ihw_sorts");
        if (launch_ihw_sorts(d_pvalue, d_group, fold, d, r.w, c->stream)) return fail(c, CHICDIFF_E_HIP, "%s: sort failed", who);
    }
    {
        Scope t(c, "ihw_hulls");
        if (launch_ihw_hulls(d, r.w, c->stream)) return fail(c, CHICDIFF_E_HIP, "%s: scan failed", who);
    }
    {
        Scope t(c, "ihw_merge");
        if (launch_ihw_merge(d, r.w, c->stream)) return fail(c, CHICDIFF_E_HIP, "%s: scan failed", who);
    }
    uint32_t total = 0;
    HIPCHK(c, hipMemcpyAsync(&r.h, r.w.dev, sizeof r.h, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipMemcpyAsync(&total, r.w.segoff + (size_t)d.nfolds * d.nb_cap, sizeof total, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    HIPCHK(c, hipGetLastError());
    r.total = total;
    const IhwDev &h = r.h;
    if (h.bad_p != ~0ull) {
        double v = 0.0;
        HIPCHK(c, hipMemcpy(&v, d_pvalue + h.bad_p, sizeof v, hipMemcpyDeviceToHost));
        return fail(c, CHICDIFF_E_INVALID, "%s: pvalue[%llu] = %g is outside [0, 1]", who, h.bad_p, v);
    }
    if (h.bad_cov != ~0ull) return fail(c, CHICDIFF_E_INVALID, "%s: covariate[%llu] is NaN on a kept row (its p-value is not NaN)", who, h.bad_cov);
    if (h.m == 0) return fail(c, CHICDIFF_E_INVALID, "%s: no kept row (every p-value is NaN)", who);
    if (h.nbins > h.m) return fail(c, CHICDIFF_E_INVALID, "%s: nbins = %u exceeds the %u kept rows", who, h.nbins, h.m);
    if (!h.ok || r.total < 1) return fail(c, CHICDIFF_E_HIP, "%s: the device reported no verdict", who);
    return CHICDIFF_OK;
}

}  // namespace

extern "C" int chicdiff_hip_ihw_caps(int32_t *max_bins, int32_t *max_folds, int32_t *auto_max_bins, int32_t *chunk_lens, int32_t cap,
                                     int32_t *nchunk_lens) {
    if (max_bins) *max_bins = kIhwMaxBins;
    if (max_folds) *max_folds = kIhwMaxFolds;
    if (auto_max_bins) *auto_max_bins = kIhwAutoMaxBins;
    const int k = (int)(sizeof kIhwChunkLens / sizeof kIhwChunkLens[0]);
    if (nchunk_lens) *nchunk_lens = k;
    for (int i = 0; chunk_lens && i < k && i < cap; i++) chunk_lens[i] = kIhwChunkLens[i];
    return CHICDIFF_OK;
}

extern "C" int chicdiff_hip_ihw_train_dev(chicdiff_hip_ctx *c, const double *d_pvalue, const double *d_covariate, int64_t n, double alpha,
                                          int32_t nbins, int32_t nfolds, uint64_t seed, int32_t *d_group, int32_t *d_fold,
                                          double *weights_host, chicdiff_ihw_info *info) {
    if (!c) return CHICDIFF_E_INVALID;
    if (!weights_host || !info) return fail(c, CHICDIFF_E_INVALID, "ihw_train: bad arguments (a NULL pointer)");
    if (!(alpha > 0.0 && alpha < 1.0)) return fail(c, CHICDIFF_E_INVALID, "ihw_train: alpha = %g (0 < alpha < 1)", alpha);
    timing_reset(c);
    IhwRun r;
    if (int rc = ihw_knots(c, "ihw_train", d_pvalue, d_covariate, n, nbins, nfolds, seed, info->chunk_len, d_group, d_fold, r)) return rc;
    if (int rc = ensure_io(c, ihw_seg_bytes(r.d, r.total), 0)) return rc;
    IhwSeg s;
    ihw_seg_carve(r.d, r.total, c->io_dev, s);
    const int nb = (int)r.h.nbins;
    {
        Scope t(c, "ihw_sweep");
        if (launch_ihw_sweep(r.d, r.w, s, r.total, nb, alpha, c->stream)) return fail(c, CHICDIFF_E_HIP, "ihw_train: sort failed");
    }
    double TH[2 * kIhwMaxFolds];
    uint32_t nsegf[kIhwMaxFolds];
    HIPCHK(c, hipMemcpyAsync(weights_host, s.w, sizeof(double) * (size_t)nb * nfolds, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipMemcpyAsync(TH, s.TH, sizeof(double) * 2 * nfolds, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipMemcpyAsync(nsegf, s.nsegf, sizeof(uint32_t) * nfolds, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    HIPCHK(c, hipGetLastError());
    timing_collect(c);
    info->m = r.h.m;
    info->nbins = nb;
    info->nfolds = nfolds;
    info->chunk_len = r.d.L;
    for (int f = 0; f < kIhwMaxFolds; f++) {
        info->nseg[f] = f < nfolds ? (int64_t)nsegf[f] : 0;
        info->T[f] = f < nfolds ? TH[2 * f] : 0.0;
        info->H[f] = f < nfolds ? TH[2 * f + 1] : 0.0;
    }
    return CHICDIFF_OK;
}

extern "C" int chicdiff_hip_selftest_ihw_knots_dev(chicdiff_hip_ctx *c, const double *d_pvalue, const double *d_covariate, int64_t n,
                                                   int32_t nbins, int32_t nfolds, uint64_t seed, int32_t chunk_len, int64_t cap,
                                                   int64_t *ptr_host, double *x_host, int32_t *c_host, int32_t *nbins_host,
                                                   int64_t *nknots_host) {
    if (!c) return CHICDIFF_E_INVALID;
    if (!nbins_host || !nknots_host || cap < 0 || (cap > 0 && (!ptr_host || !x_host || !c_host)))
        return fail(c, CHICDIFF_E_INVALID, "selftest_ihw_knots: bad arguments");
    *nbins_host = 0;
    *nknots_host = 0;
    timing_reset(c);
    IhwRun r;
    const size_t col = align256(sizeof(int32_t) * (size_t)(n > 0 ? n : 1));
    if (n >= 1 && n < (1ll << 31))
        if (int rc = ensure_io(c, col, 0)) return rc;
    if (int rc = ihw_knots(c, "selftest_ihw_knots", d_pvalue, d_covariate, n, nbins, nfolds, seed, chunk_len, (int32_t *)c->io_dev, nullptr, r)) return rc;
    timing_collect(c);
    const int nb = (int)r.h.nbins;
    const int64_t Q = (int64_t)nfolds * nb, nk = r.total + Q;
    *nbins_host = nb;
    *nknots_host = nk;
    if (cap < nk) return cap == 0 ? CHICDIFF_OK : fail(c, CHICDIFF_E_INVALID, "selftest_ihw_knots: room for %lld knots, %lld needed", (long long)cap, (long long)nk);
    const size_t pb = align256(sizeof(int64_t) * (size_t)(Q + 1)), xb = align256(sizeof(double) * (size_t)nk);
    if (int rc = ensure_io(c, pb + xb + align256(sizeof(int32_t) * (size_t)nk), 0)) return rc;
    int64_t *dp = (int64_t *)c->io_dev;
    double *dx = (double *)(c->io_dev + pb);
    int32_t *dc = (int32_t *)(c->io_dev + pb + xb);
    launch_ihw_knots_out(r.d, r.w, nb, dp, dx, dc, c->stream);
    HIPCHK(c, hipMemcpyAsync(ptr_host, dp, sizeof(int64_t) * (size_t)(Q + 1), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipMemcpyAsync(x_host, dx, sizeof(double) * (size_t)nk, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipMemcpyAsync(c_host, dc, sizeof(int32_t) * (size_t)nk, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    HIPCHK(c, hipGetLastError());
    return CHICDIFF_OK;
}

// the exact knot test as compiled for the host, on arrays of triples: sign[i] = +1 (b is a knot between a and c), 0 (collinear) or -1
extern "C" int chicdiff_hip_selftest_ihw_orient(const double *ax, const int32_t *ac, const double *bx, const int32_t *bc, const double *cx,
                                                const int32_t *cc, int64_t n, int32_t *sign) {
    if (n < 0 || (n > 0 && (!ax || !ac || !bx || !bc || !cx || !cc || !sign))) return CHICDIFF_E_INVALID;
    for (int64_t i = 0; i < n; i++) sign[i] = ihw_orient(ax[i], (uint32_t)ac[i], bx[i], (uint32_t)bc[i], cx[i], (uint32_t)cc[i]);
    return CHICDIFF_OK;
}
