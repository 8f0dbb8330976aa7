// selftest_api.hip — exports of the parity and self tests: device math, the dispersion objective, host statements of device rules.
#include "ctx.h"

// small extra export used by the parity tests: p = 2*pnorm(-|stat|) on device (Cody, as R)
extern "C" int chicdiff_hip_wald_pvalues_dev(chicdiff_hip_ctx *c, const double *d_stat, int64_t n, double *d_p) {
    if (!c) return CHICDIFF_E_INVALID;
    if (!d_stat || !d_p || n < 0) return fail(c, CHICDIFF_E_INVALID, "wald_pvalues: bad arguments");
    HIPCHK(c, hipSetDevice(c->device));
    if (n > 0) launch_pvalues(d_stat, n, d_p, c->stream);
    HIPCHK(c, hipStreamSynchronize(c->stream));
    return CHICDIFF_OK;
}

// device-math self test: op 0 flog, 1 tlog (table), 2 rcp, 3 lgamma, 4 digamma, 5 2*pnorm(-|x|), 6 / 7 raw v_rcp_f64 (+ one Newton step), 8 texp (table), 9 qnorm (AS 241)
extern "C" int chicdiff_hip_selftest_math_dev(chicdiff_hip_ctx *c, int32_t op, const double *d_x, int64_t n, double *d_out) {
    if (!c) return CHICDIFF_E_INVALID;
    if (!d_x || !d_out || n < 0 || op < 0 || op > 9) return fail(c, CHICDIFF_E_INVALID, "selftest_math: bad arguments");
    HIPCHK(c, hipSetDevice(c->device));
    if (n > 0) launch_math_selftest(op, d_x, n, d_out, c->stream);
    HIPCHK(c, hipStreamSynchronize(c->stream));
    return CHICDIFF_OK;
}

// landau_tail (devmath.h) as the "hmp" overlap kernel calls it
extern "C" int chicdiff_hip_selftest_landau_dev(chicdiff_hip_ctx *c, const double *d_z, int64_t n, double *d_out) {
    if (!c) return CHICDIFF_E_INVALID;
    if (!d_z || !d_out || n < 0) return fail(c, CHICDIFF_E_INVALID, "selftest_landau: bad arguments");
    HIPCHK(c, hipSetDevice(c->device));
    if (n > 0) launch_landau_selftest(d_z, n, d_out, c->stream);
    HIPCHK(c, hipStreamSynchronize(c->stream));
    return CHICDIFF_OK;
}

// building blocks with a second argument / a second result (header: the op numbers)
extern "C" int chicdiff_hip_selftest_math3_dev(chicdiff_hip_ctx *c, int32_t op, const double *d_x, const double *d_y, int64_t n, double *d_out,
                                               double *d_out2) {
    if (!c) return CHICDIFF_E_INVALID;
    if (!d_x || !d_y || !d_out || !d_out2 || n < 0 || op < 10 || op > 18) return fail(c, CHICDIFF_E_INVALID, "selftest_math3: bad arguments");
    HIPCHK(c, hipSetDevice(c->device));
    if (n > 0) launch_math3_selftest(op, d_x, d_y, n, c->d_logfact, d_out, d_out2, c->stream);
    HIPCHK(c, hipStreamSynchronize(c->stream));
    return CHICDIFF_OK;
}

// the dispersion objective at chosen points: the fit's own prep, then objective_probe_kernel (disp_kernels.hip)
extern "C" int chicdiff_hip_selftest_objective_dev(chicdiff_hip_ctx *c, const int32_t *d_counts, const double *d_nf, int64_t n, int32_t S,
                                                   const int32_t *group, const chicdiff_nbglm_opts *opts, const double *d_log_alpha, int32_t K,
                                                   const double *d_prior_mean, double prior_var, int32_t live_rows, double *d_lp,
                                                   double *d_dlp, double *d_alpha, double *d_mu, int32_t *lanes_per_row) {
    if (!c) return CHICDIFF_E_INVALID;
    FitDims d;
    if (!d_counts || !d_nf || !d_log_alpha || !d_lp || !d_dlp || !d_alpha || !d_mu || K < 1 || live_rows < 0 || live_rows > 64 ||
        (d_prior_mean && !(prior_var > 0)))
        return fail(c, CHICDIFF_E_INVALID, "selftest_objective: bad arguments");
    if (int rc = check_counts_group(c, n, S, group, d)) return rc;
    if (int rc = check_opts(c, opts)) return rc;
    HIPCHK(c, hipSetDevice(c->device));
    if (int rc = ensure_workspace(c, n, S)) return rc;
    const Opts o = make_opts(c, opts, S);
    HIPCHK(c, hipMemsetAsync(c->w.sc, 0, align256(sizeof(FitScalars)) + kQueueBytes + kBarrierBytes, c->stream));
    launch_prep(d_counts, const_cast<double *>(d_nf), d, c->w, o, c->stream);  // (not fused: nf is read, never written)
    ObjectiveProbe pb{d_log_alpha, K, d_prior_mean, d_prior_mean ? 1.0 / prior_var : 0.0, live_rows, d_lp, d_dlp, d_alpha, d_mu};
    const int lanes = launch_objective_probe(d, c->w, o, pb, c->stream);
    HIPCHK(c, hipStreamSynchronize(c->stream));
    if (lanes < 0) return fail(c, CHICDIFF_E_INVALID, "selftest_objective: the line search has no samples-across-lanes layout for %d live rows at S = %d", live_rows, S);
    HIPCHK(c, hipGetLastError());
    if (lanes_per_row) *lanes_per_row = lanes;
    return CHICDIFF_OK;
}

// the fit's global stage (fit_api.hip global_stage) on the caller's columns: the workspace columns are filled from them, the stage runs
// as in a pass of a fit, and what a fit does with the verdict of a failed parametric trend (fit_dev_impl) is done here the same way
extern "C" int chicdiff_hip_selftest_global_stage_dev(chicdiff_hip_ctx *c, const double *d_baseMean, const double *d_dispGeneEst,
                                                      const int32_t *d_allZero, int64_t n, int32_t S, int32_t p, const chicdiff_nbglm_opts *opts,
                                                      double *d_dispFit, double *d_resid, double *hist40, int32_t *lf_nv, double *lf_x,
                                                      double *lf_h, double *lf_f, double *lf_d, chicdiff_nbglm_scalars *scalars) {
    if (!c) return CHICDIFF_E_INVALID;
    if (!d_baseMean || !d_dispGeneEst || !d_allZero || !d_dispFit || !d_resid || !hist40 || !lf_nv || !lf_x || !lf_h || !lf_f || !lf_d || !scalars ||
        n < 1 || n > 2147483647ll || S < 2 || S > kMaxS || p < 1 || p > 2 || S <= p)
        return fail(c, CHICDIFF_E_INVALID, "selftest_global_stage: bad arguments");
    if (c->allreduce) return fail(c, CHICDIFF_E_INVALID, "selftest_global_stage: single rank only");
    if (int rc = check_opts(c, opts)) return rc;
    HIPCHK(c, hipSetDevice(c->device));
    if (int rc = ensure_workspace(c, n, S)) return rc;
    FitDims d{};
    d.n = n;
    d.S = S;
    d.p = p;
    d.nB = p == 2 ? S / 2 : 0;  // (the stage reads n, S and p alone)
    d.nA = S - d.nB;
    Opts o = make_opts(c, opts, S);
    FitWork &w = c->w;
    hipStream_t st = c->stream;
    LfTree tree;
    c->refits = 0;
    for (;;) {
        c->tg_total = 0;
        HIPCHK(c, hipMemsetAsync(w.sc, 0, align256(sizeof(FitScalars)) + kQueueBytes + kBarrierBytes, st));
        HIPCHK(c, hipMemcpyAsync(w.baseMean, d_baseMean, sizeof(double) * (size_t)n, hipMemcpyDeviceToDevice, st));
        HIPCHK(c, hipMemcpyAsync(w.dispGene, d_dispGeneEst, sizeof(double) * (size_t)n, hipMemcpyDeviceToDevice, st));
        HIPCHK(c, hipMemcpyAsync(w.allZero, d_allZero, sizeof(int32_t) * (size_t)n, hipMemcpyDeviceToDevice, st));
        HIPCHK(c, hipMemsetAsync(w.dispFit, 0xff, sizeof(double) * (size_t)n, st));  // NaN: only a local trend writes the column in this stage
        if (int rc = global_stage(c, d, o, c->host.select_all_rounds != 0, &tree)) return rc;
        HIPCHK(c, hipMemcpyAsync(c->h_sc, w.sc, sizeof(FitScalars), hipMemcpyDeviceToHost, st));
        HIPCHK(c, hipStreamSynchronize(st));
        HIPCHK(c, hipGetLastError());
        if (c->h_sc->failed == 3) {  // the persistent kernel's grid barrier timed out: one launch per pass, as fit_dev_impl answers it
            if (c->no_persistent_trend) return fail(c, CHICDIFF_E_HIP, "trend fit: grid barrier timed out");
            c->no_persistent_trend = true;
        } else if (substitute_local_trend(c, o)) {
            o.fit_type = 2;
        } else
            break;
        c->refits++;
    }
    const bool mc = prior_by_simulation(d, o);
    double *d_hist = resid_hist_of(w);
    if (mc) HIPCHK(c, hipMemcpyAsync(hist40, d_hist, sizeof(double) * kPmcBins, hipMemcpyDeviceToHost, st));
    else memset(hist40, 0, sizeof(double) * kPmcBins);
    HIPCHK(c, hipMemcpyAsync(d_dispFit, w.dispFit, sizeof(double) * (size_t)n, hipMemcpyDeviceToDevice, st));
    HIPCHK(c, hipMemcpyAsync(d_resid, w.resid, sizeof(double) * (size_t)n, hipMemcpyDeviceToDevice, st));
    HIPCHK(c, hipStreamSynchronize(st));
    const FitScalars *s = c->h_sc;
    *lf_nv = s->trend_local ? tree.nv : 0;
    for (int i = 0; i < *lf_nv; i++) { lf_x[i] = tree.x[i]; lf_h[i] = tree.h[i]; lf_f[i] = tree.f[i]; lf_d[i] = tree.d[i]; }
    memset(scalars, 0, sizeof *scalars);
    int status = 0;
    if (s->failed) status |= CHICDIFF_ST_TREND_FAILED;
    if (s->trend_local) status |= CHICDIFF_ST_TREND_LOCAL;
    if (mc) status |= CHICDIFF_ST_PRIORVAR_MC;
    scalars->trendCoef[0] = s->coefs[0];
    scalars->trendCoef[1] = s->coefs[1];
    scalars->varLogDispEsts = s->varLogDispEsts;
    scalars->dispPriorVar = s->dispPriorVar;
    scalars->sumDeviance = NAN;
    scalars->trendOuterIter = s->outer_it;
    scalars->status = status;
    return CHICDIFF_OK;
}

// launch_resid_hist (resid_hist_kernel, pmc_bin) on the caller's residual column
extern "C" int chicdiff_hip_selftest_resid_hist_dev(chicdiff_hip_ctx *c, const double *d_resid, int64_t n, double *hist40) {
    if (!c) return CHICDIFF_E_INVALID;
    if (!d_resid || !hist40 || n < 1 || n > 2147483647ll) return fail(c, CHICDIFF_E_INVALID, "selftest_resid_hist: bad arguments");
    HIPCHK(c, hipSetDevice(c->device));
    if (int rc = ensure_workspace(c, 1, 2)) return rc;
    FitDims d{};
    d.n = n;
    FitWork wm = c->w;
    wm.resid = const_cast<double *>(d_resid);  // (read only)
    double *d_hist = resid_hist_of(c->w);
    launch_resid_hist(d, wm, d_hist, c->stream);
    HIPCHK(c, hipMemcpyAsync(hist40, d_hist, sizeof(double) * kPmcBins, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    HIPCHK(c, hipGetLastError());
    return CHICDIFF_OK;
}

// host-side self tests of the simulation-matched prior variance (no device involved)
extern "C" int chicdiff_hip_selftest_r_random(int32_t kind, uint32_t seed, double a, double b, int64_t n, double *out) {
    if (!out || n < 0 || kind < 0 || kind > 3) return CHICDIFF_E_INVALID;
    if (kind == 3 && !(a > 0 && b > 0)) return CHICDIFF_E_INVALID;
    RStream r(seed);
    for (int64_t i = 0; i < n; i++) out[i] = kind == 0 ? r.unif() : kind == 1 ? r.norm() : kind == 2 ? r.expo() : r.gamma(a, b);
    return CHICDIFF_OK;
}
// the gene-wise schedule's class function (common.h), evaluated on the host: class index of each score, and in `bounds` (7 values) the
// first class index that is not dealt out statically for 0 .. 6 of the half-decade classes
extern "C" int chicdiff_hip_selftest_sched_class(int32_t mode, double min_disp, const double *alpha_init, const double *group_mean, int64_t n,
                                                 int32_t *cls_out, int32_t *bounds) {
    if (n < 0 || (n > 0 && (!alpha_init || !group_mean || !cls_out)) || mode < 1 || mode > 4) return CHICDIFF_E_INVALID;
    for (int64_t i = 0; i < n; i++) cls_out[i] = cd::sched_class(alpha_init[i], group_mean[i], min_disp, mode);
    if (bounds) for (int a = 0; a <= 6; a++) bounds[a] = cd::sched_classes_a(a, mode);
    return CHICDIFF_OK;
}
// the value bins of the direct size-factor select (common.h: sf_bin, sf_sub_bin), evaluated on the host: bins per column for S samples
// (*nbins_out), the bin of each x, and — sub_out given — its sub-bin inside bin `sub_of`
extern "C" int chicdiff_hip_selftest_sf_bin(int32_t S, const double *x, int64_t n, int32_t *nbins_out, int32_t *bin_out, int32_t sub_of,
                                            int32_t *sub_out) {
    if (S < 1 || S > cd::kSfMaxS || n < 0 || (n > 0 && (!x || !bin_out))) return CHICDIFF_E_INVALID;
    const int nb = cd::sf_bins(S);
    if (nbins_out) *nbins_out = nb;
    for (int64_t i = 0; i < n; i++) {
        bin_out[i] = cd::sf_bin(x[i], nb);
        if (sub_out) sub_out[i] = cd::sf_sub_bin(x[i], nb, sub_of);
    }
    return CHICDIFF_OK;
}
// the claim rule of the gene-wise line search's two-ended queue (common.h: queue_claim, filler_claims, filler_stop_f), evaluated on the host
extern "C" int chicdiff_hip_selftest_queue_claim(uint64_t old, int32_t back, uint32_t chunks, uint32_t first_back, int32_t stop_percent, int32_t claimed,
                                                 uint32_t *chunk_out, int32_t *again_out) {
    uint32_t chunk = 0;
    const bool valid = cd::queue_claim(old, back != 0, chunks, chunk);
    if (chunk_out) *chunk_out = chunk;
    if (again_out) *again_out = cd::filler_claims(claimed != 0, old, chunks, first_back, cd::filler_stop_f(stop_percent, chunks, first_back));
    return valid ? 1 : 0;
}
// the words of the persistent trend kernel's exchange (fit_state.h: xchg_pack, xchg_unpack, xchg_accept), evaluated on the host
extern "C" int chicdiff_hip_selftest_trend_exchange(int32_t op, uint32_t tag, int64_t n, double *x, uint64_t *words, int32_t *accept) {
    if (op < 0 || op > 2 || n < 0 || (n > 0 && (!words || (op != 2 && !x) || (op == 2 && !accept)))) return CHICDIFF_E_INVALID;
    for (int64_t i = 0; i < n; i++) {
        if (op == 0) cd::xchg_pack(x[i], tag, &words[2 * i], &words[2 * i + 1]);
        else if (op == 1) {
            x[i] = cd::xchg_unpack(words[2 * i], words[2 * i + 1]);
            if (accept) accept[i] = cd::xchg_accept(words[2 * i], tag) && cd::xchg_accept(words[2 * i + 1], tag);
        } else
            accept[i] = cd::xchg_accept(words[i], tag);
    }
    return CHICDIFF_OK;
}
extern "C" int chicdiff_hip_selftest_prior_mc(int32_t df, const double *hist40, double *dens_out, double *prior_var_out) {
    if (df < 1 || df > 3) return CHICDIFF_E_INVALID;
    const PmcTable &t = pmc_table(df);
    if (dens_out) memcpy(dens_out, t.dens, sizeof t.dens);
    if (prior_var_out) {
        if (!hist40) return CHICDIFF_E_INVALID;
        *prior_var_out = pmc_prior_var(hist40, t);
    }
    return CHICDIFF_OK;
}
