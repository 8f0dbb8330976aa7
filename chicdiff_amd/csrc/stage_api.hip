// stage_api.hip — entry points of the stages around the fit: one stream, one synchronisation per call.
#include "ctx.h"
#include "philox.h"
#include "ru_window.h"

extern "C" {

int chicdiff_hip_window_sums_dev(chicdiff_hip_ctx *c, const int32_t *d_fragN, const double *d_fragFM, int64_t nfrag,
                                 int32_t S, const int64_t *d_region_ptr, int64_t n, int32_t *d_N, double *d_FM) {
    if (!c) return CHICDIFF_E_INVALID;
    if (!d_region_ptr || n < 1 || S < 1 || (d_fragN && !d_N) || (d_fragFM && !d_FM))
        return fail(c, CHICDIFF_E_INVALID, "window_sums: bad arguments");
    HIPCHK(c, hipSetDevice(c->device));
    timing_reset(c);
    {
        Scope t(c, "window_sums");
        launch_window_sums(d_fragN, d_fragFM, nfrag, S, d_region_ptr, n, d_N, d_FM, c->stream);
    }
    HIPCHK(c, hipStreamSynchronize(c->stream));
    timing_collect(c);
    return CHICDIFF_OK;
}

int chicdiff_hip_count_join_dev(chicdiff_hip_ctx *c, const int32_t *d_ru_bait, const int32_t *d_ru_oe, int64_t nru,
                                const int64_t *d_keys, const int32_t *d_vals, int64_t nkeys, int32_t *d_out) {
    if (!c) return CHICDIFF_E_INVALID;
    if (!d_ru_bait || !d_ru_oe || !d_out || nru < 0 || nkeys < 0 || (nkeys > 0 && (!d_keys || !d_vals)))
        return fail(c, CHICDIFF_E_INVALID, "count_join: bad arguments");
    HIPCHK(c, hipSetDevice(c->device));
    timing_reset(c);
    if (nru > 0) {
        if (int rc = ensure_aux(c, count_join_scratch_bytes(nkeys))) return rc;
        Scope t(c, "count_join");
        launch_count_join(d_ru_bait, d_ru_oe, nru, d_keys, d_vals, nkeys, d_out, c->aux, c->stream);
    }
    HIPCHK(c, hipStreamSynchronize(c->stream));
    timing_collect(c);
    return CHICDIFF_OK;
}

}  // extern "C"

// a3 — per-fragment background (Bmean, Tmean, FullMean) for every RU row and replicate
extern "C" int chicdiff_hip_fragment_background_dev(chicdiff_hip_ctx *c, const int32_t *d_bait, const int32_t *d_oe, int64_t nru,
                                                    int32_t id_min, int32_t nid, const int64_t *d_midsum, int32_t S,
                                                    const double *d_sj, const double *d_si, const int32_t *d_tblb,
                                                    const int32_t *d_tlb, const double *d_T, int32_t ntblb, int32_t ntlb,
                                                    const double *distfun_host, double *d_bmean, double *d_tmean,
                                                    double *d_fullmean) {
    if (!c) return CHICDIFF_E_INVALID;
    if (!d_bait || !d_oe || !d_midsum || !d_sj || !d_si || !d_tblb || !d_tlb || !d_T || !distfun_host || nru < 0 || nid < 1 ||
        S < 1 || S > kMaxS || ntblb < 1 || ntlb < 1)
        return fail(c, CHICDIFF_E_INVALID, "fragment_background: bad arguments");
    HIPCHK(c, hipSetDevice(c->device));
    int rc = ensure_aux(c, sizeof(double) * 10 * kMaxS);  // (the context's scratch: no allocation per call once warm)
    if (rc) return rc;
    double *d_df = reinterpret_cast<double *>(c->aux);
    hipError_t e = hipMemcpyAsync(d_df, distfun_host, sizeof(double) * 10 * S, hipMemcpyHostToDevice, c->stream);
    timing_reset(c);
    if (e == hipSuccess && nru > 0) {
        Scope t(c, "fragment_background");
        launch_fragment_background(d_bait, d_oe, nru, id_min, nid, d_midsum, S, d_sj, d_si, d_tblb, d_tlb, d_T, ntblb, ntlb, d_df,
                                   d_bmean, d_tmean, d_fullmean, c->stream);
    }
    if (e == hipSuccess) e = hipStreamSynchronize(c->stream);
    timing_collect(c);
    if (e != hipSuccess) return fail(c, CHICDIFF_E_HIP, "fragment_background: %s", hipGetErrorString(e));
    return CHICDIFF_OK;
}

// ---- f1 / f3 / f4 (post_kernels.hip) ------------------------------------------------------------------------
extern "C" int chicdiff_hip_bh_adjust_dev(chicdiff_hip_ctx *c, const double *d_p, int64_t n, double *d_padj) {
    if (!c) return CHICDIFF_E_INVALID;
    if (n < 0 || n >= (1ll << 32) || (n > 0 && (!d_p || !d_padj))) return fail(c, CHICDIFF_E_INVALID, "bh_adjust: bad arguments");
    if (n == 0) return CHICDIFF_OK;
    HIPCHK(c, hipSetDevice(c->device));
    int rc = ensure_aux(c, bh_workspace_bytes(n));
    if (rc) return rc;
    timing_reset(c);
    {
        Scope t(c, "bh_adjust");
        if (launch_bh_adjust(d_p, n, d_padj, c->aux, c->stream)) return fail(c, CHICDIFF_E_HIP, "bh_adjust: sort/scan failed");
    }
    HIPCHK(c, hipStreamSynchronize(c->stream));
    timing_collect(c);
    return CHICDIFF_OK;
}

extern "C" int chicdiff_hip_ihw_apply_dev(chicdiff_hip_ctx *c, const double *d_avDist, const double *d_pvalue, int64_t n,
                                          const double *breaks_host, const double *avWeights_host, int32_t ngroups,
                                          int32_t *d_group, double *d_weight, double *d_wp, double *d_wpadj) {
    if (!c) return CHICDIFF_E_INVALID;
    if (!d_avDist || !d_pvalue || !breaks_host || !avWeights_host || !d_wpadj || n < 1 || n >= (1ll << 32) || ngroups < 1 || ngroups > 256)
        return fail(c, CHICDIFF_E_INVALID, "ihw_apply: bad arguments");
    for (int k = 0; k < ngroups; k++)
        if (!(breaks_host[k] < breaks_host[k + 1])) return fail(c, CHICDIFF_E_INVALID, "ihw_apply: breaks must be strictly ascending ('breaks' are not unique)");
    HIPCHK(c, hipSetDevice(c->device));
    const size_t bhb = bh_workspace_bytes(n), ihwb = align256(ihw_workspace_bytes()), col = align256(sizeof(double) * (size_t)n);
    int rc = ensure_aux(c, bhb + ihwb + 2 * col);
    if (rc) return rc;
    double *partials = (double *)(c->aux + bhb);
    double *weight = d_weight ? d_weight : (double *)(c->aux + bhb + ihwb);
    double *wp = d_wp ? d_wp : (double *)(c->aux + bhb + ihwb + col);
    timing_reset(c);
    {
        Scope t(c, "ihw_apply");
        launch_ihw_apply(d_avDist, d_pvalue, n, breaks_host, avWeights_host, ngroups, d_group, weight, wp, partials, c->stream);
        if (launch_bh_adjust(wp, n, d_wpadj, c->aux, c->stream)) return fail(c, CHICDIFF_E_HIP, "ihw_apply: sort/scan failed");
    }
    HIPCHK(c, hipStreamSynchronize(c->stream));
    timing_collect(c);
    return CHICDIFF_OK;
}

extern "C" int chicdiff_hip_region_universe_count_dev(chicdiff_hip_ctx *c, const int32_t *d_bait, const int32_t *d_oe, int64_t n,
                                                      int32_t RUexpand, const int32_t *d_chr_of, int32_t maxfrag,
                                                      int64_t *d_region_ptr, int32_t *d_minOE, int32_t *d_maxOE,
                                                      int64_t *total_host) {
    if (!c) return CHICDIFF_E_INVALID;
    if (!d_bait || !d_oe || !d_chr_of || !d_region_ptr || !total_host || n < 1 || RUexpand < 0 || RUexpand > (1 << 20) || maxfrag < 1)
        return fail(c, CHICDIFF_E_INVALID, "region_universe: bad arguments");
    if (maxfrag > kRuMaxFrag)
        return fail(c, CHICDIFF_E_INVALID, "region_universe: maxfrag = %d (1 <= maxfrag < 2^30: the window's counters are 32-bit)", (int)maxfrag);
    HIPCHK(c, hipSetDevice(c->device));
    const size_t scan = ru_scan_bytes(n);
    int rc = ensure_aux(c, 256 + scan);
    if (rc) return rc;
    int *bad = (int *)c->aux;
    timing_reset(c);
    {
        Scope t(c, "region_universe");
        if (launch_ru_count(d_bait, d_oe, n, RUexpand, d_chr_of, maxfrag, d_region_ptr, d_minOE, d_maxOE, bad, c->aux + 256, scan, c->stream))
            return fail(c, CHICDIFF_E_HIP, "region_universe: scan failed");
    }
    int h_bad = 0;
    HIPCHK(c, hipMemcpyAsync(&h_bad, bad, sizeof(int), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipMemcpyAsync(total_host, d_region_ptr + n, sizeof(int64_t), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    timing_collect(c);
    if (h_bad) return fail(c, CHICDIFF_E_INVALID, "region_universe: Invalid parameters (a peak with baitID == oeID)");
    return CHICDIFF_OK;
}

extern "C" int chicdiff_hip_region_universe_fill_dev(chicdiff_hip_ctx *c, const int32_t *d_bait, const int32_t *d_oe, int64_t n,
                                                     int32_t RUexpand, const int32_t *d_chr_of, int32_t maxfrag,
                                                     const int64_t *d_region_ptr, int32_t *d_ru_bait, int32_t *d_ru_region,
                                                     int32_t *d_ru_oe) {
    if (!c) return CHICDIFF_E_INVALID;
    if (!d_bait || !d_oe || !d_chr_of || !d_region_ptr || !d_ru_bait || !d_ru_region || !d_ru_oe || n < 1 || RUexpand < 0 || maxfrag < 1)
        return fail(c, CHICDIFF_E_INVALID, "region_universe: bad arguments");
    if (maxfrag > kRuMaxFrag)
        return fail(c, CHICDIFF_E_INVALID, "region_universe: maxfrag = %d (1 <= maxfrag < 2^30: the window's counters are 32-bit)", (int)maxfrag);
    HIPCHK(c, hipSetDevice(c->device));
    timing_reset(c);
    {
        Scope t(c, "region_universe");
        launch_ru_fill(d_bait, d_oe, n, RUexpand, d_chr_of, maxfrag, d_region_ptr, d_ru_bait, d_ru_region, d_ru_oe, c->stream);
    }
    HIPCHK(c, hipStreamSynchronize(c->stream));
    timing_collect(c);
    return CHICDIFF_OK;
}

// both steps in one call (round 5): the caller gives room for the upper bound n max(2 RUexpand + 1, 2) rows, so that nothing on the host
// stands between the scan and the fill — one synchronisation and one read-back instead of two of each
extern "C" int chicdiff_hip_region_universe_dev(chicdiff_hip_ctx *c, const int32_t *d_bait, const int32_t *d_oe, int64_t n, int32_t RUexpand,
                                                const int32_t *d_chr_of, int32_t maxfrag, int64_t *d_region_ptr, int32_t *d_minOE,
                                                int32_t *d_maxOE, int32_t *d_ru_bait, int32_t *d_ru_region, int32_t *d_ru_oe,
                                                int64_t capacity, int64_t *total_host) {
    if (!c) return CHICDIFF_E_INVALID;
    if (!d_bait || !d_oe || !d_chr_of || !d_region_ptr || !d_ru_bait || !d_ru_region || !d_ru_oe || !total_host || n < 1 || RUexpand < 0 ||
        RUexpand > (1 << 20) || maxfrag < 1)
        return fail(c, CHICDIFF_E_INVALID, "region_universe: bad arguments");
    if (maxfrag > kRuMaxFrag)
        return fail(c, CHICDIFF_E_INVALID, "region_universe: maxfrag = %d (1 <= maxfrag < 2^30: the window's counters are 32-bit)", (int)maxfrag);
    // rows per peak: (oe - s):(oe + s) = 2 s + 1 — or, for RUexpand = 0 and a peak right beside its bait, R's DESCENDING (bait + 2):(oe + 0): two
    const int64_t per_peak = RUexpand > 0 ? 2 * (int64_t)RUexpand + 1 : 2;
    if (capacity < n * per_peak)
        return fail(c, CHICDIFF_E_INVALID, "region_universe: room for n max(2 RUexpand + 1, 2) = %lld rows needed, %lld given",
                    (long long)(n * per_peak), (long long)capacity);
    HIPCHK(c, hipSetDevice(c->device));
    const size_t scan = align256(ru_scan_bytes(n));
    int rc = ensure_aux(c, 256 + scan + sizeof(unsigned int) * (size_t)n);
    if (rc) return rc;
    int *bad = (int *)c->aux;
    unsigned int *masks = reinterpret_cast<unsigned int *>(c->aux + 256 + scan);  // which candidates each region keeps: counted once, read by the fill
    timing_reset(c);
    {
        Scope t(c, "region_universe");
        if (launch_ru_count(d_bait, d_oe, n, RUexpand, d_chr_of, maxfrag, d_region_ptr, d_minOE, d_maxOE, bad, c->aux + 256, scan, c->stream, masks))
            return fail(c, CHICDIFF_E_HIP, "region_universe: scan failed");
        launch_ru_fill(d_bait, d_oe, n, RUexpand, d_chr_of, maxfrag, d_region_ptr, d_ru_bait, d_ru_region, d_ru_oe, c->stream, masks);
    }
    int h_bad = 0;
    HIPCHK(c, hipMemcpyAsync(&h_bad, bad, sizeof(int), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipMemcpyAsync(total_host, d_region_ptr + n, sizeof(int64_t), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    timing_collect(c);
    if (h_bad) return fail(c, CHICDIFF_E_INVALID, "region_universe: Invalid parameters (a peak with baitID == oeID)");
    return CHICDIFF_OK;
}

// getCandidateInteractions (chicdiff.R:2068-2163): everything is enqueued behind one another; the one host stop is the read of the
// counts (and of the refusals' row numbers, which ride in the same 40 bytes)
extern "C" int chicdiff_hip_candidate_interactions_method_dev(chicdiff_hip_ctx *c, const int32_t *d_baitID, const int32_t *d_minOE,
                                                              const int32_t *d_maxOE, const double *d_p, int64_t n,
                                                              const int32_t *d_peak_baitID, const int32_t *d_peak_oeID, const double *d_scores,
                                                              int64_t npeaks, int32_t ncols, int32_t ncond1, int32_t ncond2, int32_t merged,
                                                              double score, double pvcut, double minDeltaAsinhScore, int32_t method,
                                                              int64_t pair_capacity, int32_t *d_group_peak, int64_t *d_group_ptr,
                                                              double *d_group_min_p, double *d_group_delta, int32_t *d_pair_row,
                                                              int64_t *ngroups_host, int64_t *npairs_host) {
    if (!c) return CHICDIFF_E_INVALID;
    if (ngroups_host) *ngroups_host = 0;
    if (npairs_host) *npairs_host = 0;
    if (method != CHICDIFF_CAND_MIN && method != CHICDIFF_CAND_HMP)
        return fail(c, CHICDIFF_E_INVALID, "candidate_interactions: method = %d (CHICDIFF_CAND_MIN = 0 or CHICDIFF_CAND_HMP = 1)", (int)method);
    if (!d_baitID || !d_minOE || !d_maxOE || !d_p || !d_group_peak || !d_group_ptr || !d_group_min_p || !d_group_delta || !ngroups_host ||
        !npairs_host || (pair_capacity > 0 && !d_pair_row) || pair_capacity < 0 || (npeaks > 0 && (!d_peak_baitID || !d_peak_oeID || !d_scores)))
        return fail(c, CHICDIFF_E_INVALID, "candidate_interactions: bad arguments");
    if (n < 1 || n >= (1ll << 31))
        return fail(c, CHICDIFF_E_INVALID, "candidate_interactions: n = %lld regions (1 <= n < 2^31: pair rows are int32)", (long long)n);
    if (ncols < 2) return fail(c, CHICDIFF_E_INVALID, "candidate_interactions: ncols = %d score columns (at least one per condition)", (int)ncols);
    if (npeaks < 0 || npeaks >= (1ll << 31))
        return fail(c, CHICDIFF_E_INVALID, "candidate_interactions: npeaks = %lld (0 <= npeaks < 2^31)", (long long)npeaks);
    if ((merged != 0 && merged != 1) || ncond1 < 1 || ncond2 < 1 || ncond1 + ncond2 != ncols || (merged && ncols != 2))
        return fail(c, CHICDIFF_E_INVALID, "candidate_interactions: ncond1 = %d, ncond2 = %d, merged = %d do not describe %d score columns",
                    (int)ncond1, (int)ncond2, (int)merged, (int)ncols);
    HIPCHK(c, hipSetDevice(c->device));
    if (int rc = ensure_aux(c, cand_workspace_bytes(n, npeaks))) return rc;
    CandArgs a;
    a.bait = d_baitID; a.minOE = d_minOE; a.maxOE = d_maxOE; a.p = d_p; a.n = n;
    a.peak_bait = d_peak_baitID; a.peak_oe = d_peak_oeID; a.scores = d_scores; a.npeaks = npeaks;
    a.ncols = ncols; a.ncond1 = ncond1; a.merged = merged;
    a.score = score; a.pvcut = pvcut; a.min_delta = minDeltaAsinhScore; a.method = method; a.pair_capacity = pair_capacity;
    a.group_peak = d_group_peak; a.group_ptr = d_group_ptr; a.group_min_p = d_group_min_p; a.group_delta = d_group_delta;
    a.pair_row = d_pair_row;
    const CandResult *d_res = nullptr;
    timing_reset(c);
    {
        Scope t(c, "candidates");
        if (launch_candidates(a, c->aux, c->stream, &d_res)) return fail(c, CHICDIFF_E_HIP, "candidate_interactions: sort/scan failed");
    }
    CandResult h;
    HIPCHK(c, hipMemcpyAsync(&h, d_res, sizeof h, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    HIPCHK(c, hipGetLastError());
    timing_collect(c);
    if (h.bad_region != ~0ull)
        return fail(c, CHICDIFF_E_INVALID, "candidate_interactions: region row %llu has minOE > maxOE or an NA (INT32_MIN) key: foverlaps stops on it",
                    h.bad_region);
    if (h.bad_peak_key != ~0ull)
        return fail(c, CHICDIFF_E_INVALID, "candidate_interactions: peak row %llu has baitID = oeID = INT32_MAX, which is not a fragment ID", h.bad_peak_key);
    if (h.dup_peak != ~0ull)
        return fail(c, CHICDIFF_E_INVALID, "candidate_interactions: peak row %llu repeats the (baitID, oeID) of an earlier selected row: the peak matrix "
                    "has one row per pair", h.dup_peak);
    *ngroups_host = h.ngroups;
    *npairs_host = h.npairs;
    if (h.npairs > pair_capacity)
        return fail(c, CHICDIFF_E_INVALID, "candidate_interactions: room for %lld pairs needed, %lld given (no pair was written)", h.npairs,
                    (long long)pair_capacity);
    return CHICDIFF_OK;
}

extern "C" int chicdiff_hip_candidate_interactions_dev(chicdiff_hip_ctx *c, const int32_t *d_baitID, const int32_t *d_minOE,
                                                       const int32_t *d_maxOE, const double *d_p, int64_t n, const int32_t *d_peak_baitID,
                                                       const int32_t *d_peak_oeID, const double *d_scores, int64_t npeaks, int32_t ncols,
                                                       int32_t ncond1, int32_t ncond2, int32_t merged, double score, double pvcut,
                                                       double minDeltaAsinhScore, int64_t pair_capacity, int32_t *d_group_peak,
                                                       int64_t *d_group_ptr, double *d_group_min_p, double *d_group_delta, int32_t *d_pair_row,
                                                       int64_t *ngroups_host, int64_t *npairs_host) {
    return chicdiff_hip_candidate_interactions_method_dev(c, d_baitID, d_minOE, d_maxOE, d_p, n, d_peak_baitID, d_peak_oeID, d_scores, npeaks, ncols,
                                                          ncond1, ncond2, merged, score, pvcut, minDeltaAsinhScore, CHICDIFF_CAND_MIN, pair_capacity,
                                                          d_group_peak, d_group_ptr, d_group_min_p, d_group_delta, d_pair_row, ngroups_host,
                                                          npairs_host);
}

// The seeded control draws (chicdiff.R:430-481): contact pass, draws, sort and unpack enqueued behind one another; the one host stop is
// the read of the counts (and of the refusals, which ride in the same 40 bytes)
extern "C" int chicdiff_hip_control_draws_dev(chicdiff_hip_ctx *c, const int32_t *d_ru_baitID, int64_t nru, const int64_t *d_region_ptr,
                                              const int32_t *d_minOE, const int32_t *d_maxOE, int64_t n, const int32_t *d_bmap_id,
                                              const int32_t *d_bmap_chr, int64_t nb, const int32_t *chr_min, const int32_t *chr_max,
                                              int32_t nchr, uint64_t seed, int32_t *d_ctrl_baitID, int32_t *d_ctrl_oeID,
                                              int32_t *d_max_contact, int64_t *n_regions_host, int64_t *m_host) {
    if (!c) return CHICDIFF_E_INVALID;
    if (n_regions_host) *n_regions_host = 0;
    if (m_host) *m_host = 0;
    if (!d_ru_baitID || !d_region_ptr || !d_minOE || !d_maxOE || !d_bmap_id || !d_bmap_chr || !chr_min || !chr_max || !d_ctrl_baitID ||
        !d_ctrl_oeID || !d_max_contact || !n_regions_host || !m_host || nru < 0)
        return fail(c, CHICDIFF_E_INVALID, "control_draws: bad arguments (a NULL pointer)");
    if (n < 1 || n >= (1ll << 31)) return fail(c, CHICDIFF_E_INVALID, "control_draws: n = %lld regions (1 <= n < 2^31)", (long long)n);
    if (nb < 1 || nb >= (1ll << 31)) return fail(c, CHICDIFF_E_INVALID, "control_draws: nb = %lld baits on the baitmap (1 <= nb < 2^31)", (long long)nb);
    if (nchr < 1 || nchr > CHICDIFF_CONTROL_MAX_CHR)
        return fail(c, CHICDIFF_E_INVALID, "control_draws: nchr = %d chromosomes (1 <= nchr <= %d: the capacity of the LDS tables)", (int)nchr,
                    CHICDIFF_CONTROL_MAX_CHR);
    // the chromosomes as disjoint ID ranges sorted by their first ID: how the contact pass finds a bait's chromosome
    std::vector<int32_t> order, lo, hi, code;
    for (int32_t k = 0; k < nchr; k++)
        if (chr_min[k] <= chr_max[k]) order.push_back(k);
    std::sort(order.begin(), order.end(), [&](int32_t a, int32_t b) { return chr_min[a] < chr_min[b]; });
    for (size_t j = 0; j < order.size(); j++) {
        const int32_t k = order[j];
        if (j > 0 && chr_min[k] <= hi.back())
            return fail(c, CHICDIFF_E_INVALID, "control_draws: the ID ranges of chromosome codes %d [%d, %d] and %d [%d, %d] overlap: a chromosome "
                        "must be one run of restriction-map IDs", (int)code.back(), (int)lo.back(), (int)hi.back(), (int)k, (int)chr_min[k], (int)chr_max[k]);
        lo.push_back(chr_min[k]);
        hi.push_back(chr_max[k]);
        code.push_back(k);
    }
    HIPCHK(c, hipSetDevice(c->device));
    if (int rc = ensure_aux(c, ctrl_workspace_bytes(n, nchr))) return rc;
    CtrlArgs a;
    a.ru_bait = d_ru_baitID; a.nru = nru; a.region_ptr = d_region_ptr; a.minOE = d_minOE; a.maxOE = d_maxOE; a.n = n;
    a.bmap_id = d_bmap_id; a.bmap_chr = d_bmap_chr; a.nb = nb; a.chr_min = chr_min; a.chr_max = chr_max; a.nchr = nchr; a.seed = seed;
    a.ctrl_bait = d_ctrl_baitID; a.ctrl_oe = d_ctrl_oeID; a.max_contact = d_max_contact;
    const CtrlResult *d_res = nullptr;
    timing_reset(c);
    {
        Scope t(c, "control_draws");
        if (launch_control_draws(a, lo.data(), hi.data(), code.data(), (int)code.size(), c->aux, c->stream, &d_res))
            return fail(c, CHICDIFF_E_HIP, "control_draws: copy/sort failed");
    }
    CtrlResult h;
    HIPCHK(c, hipMemcpyAsync(&h, d_res, sizeof h, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    HIPCHK(c, hipGetLastError());
    timing_collect(c);
    if (h.bad_region != ~0ull)
        return fail(c, CHICDIFF_E_INVALID, "control_draws: region_ptr[%llu .. %llu + 1] is not an ascending pair of offsets inside [0, %lld]", h.bad_region,
                    h.bad_region, (long long)nru);
    if (h.bad_bait != ~0ull)
        return fail(c, CHICDIFF_E_INVALID, "control_draws: row %llu of the baitmap has chromosome code >= nchr = %d", h.bad_bait, (int)nchr);
    if (h.n_regions == 0) return fail(c, CHICDIFF_E_INVALID, "control_draws: RU holds no non-empty region");
    if (h.cap_k != ~0ull) {  // name the draw: its bait is a function of (seed, k) that the host can restate
        const Philox4 r = control_draw_words(seed, h.cap_k, 0, 0);
        const uint64_t idx = (uint64_t)(((unsigned __int128)((uint64_t)r.w[0] | ((uint64_t)r.w[1] << 32)) * (unsigned __int128)(uint64_t)nb) >> 64);
        int32_t bait = 0, chr = -1;
        HIPCHK(c, hipMemcpy(&bait, d_bmap_id + idx, sizeof bait, hipMemcpyDeviceToHost));
        HIPCHK(c, hipMemcpy(&chr, d_bmap_chr + idx, sizeof chr, hipMemcpyDeviceToHost));
        return fail(c, CHICDIFF_E_INVALID, "control_draws: draw k = %llu (bait %d on chromosome code %d, IDs %d .. %d) found no valid distance in %d "
                    "attempts: the chromosome leaves this bait no fragment to go to", h.cap_k, (int)bait, (int)chr,
                    chr >= 0 && chr < nchr ? (int)chr_min[chr] : 0, chr >= 0 && chr < nchr ? (int)chr_max[chr] : 0, CHICDIFF_CONTROL_MAX_ATTEMPTS);
    }
    *n_regions_host = (int64_t)h.n_regions;
    *m_host = (int64_t)h.m;
    return CHICDIFF_OK;
}

// The Chicago background tables of one replicate (chicdiff.R:656-692, 538-548): init, two streaming passes and an epilogue behind one
// another; the one host stop is the read of the status word
extern "C" int chicdiff_hip_chicago_tables_dev(chicdiff_hip_ctx *c, const int32_t *d_bait, const int32_t *d_oe, const double *d_s_j,
                                               const double *d_s_i, const double *d_Tmean, const double *d_refBinMean, const int32_t *d_tblb,
                                               const int32_t *d_tlb, const int32_t *d_distbin, int64_t nrows, int32_t id_min, int32_t nid,
                                               int32_t ntblb, int32_t ntlb, int32_t ndistbin, double *d_sj, double *d_si, int32_t *d_tblb_of,
                                               int32_t *d_tlb_of, double *d_T, double *d_ref, int32_t *status_host) {
    if (!c) return CHICDIFF_E_INVALID;
    if (status_host) *status_host = 0;
    if (!d_bait || !d_oe || !d_s_j || !d_s_i || !d_Tmean || !d_refBinMean || !d_tblb || !d_tlb || !d_distbin || !d_sj || !d_si || !d_tblb_of ||
        !d_tlb_of || !d_T || !d_ref || !status_host)
        return fail(c, CHICDIFF_E_INVALID, "chicago_tables: bad arguments (a NULL pointer)");
    if (nrows < 1 || nrows >= (1ll << 32))
        return fail(c, CHICDIFF_E_INVALID, "chicago_tables: nrows = %lld (1 <= nrows < 2^32: the row index is half of a 64-bit atomic word)",
                    (long long)nrows);
    if (nid < 1) return fail(c, CHICDIFF_E_INVALID, "chicago_tables: nid = %d (an empty restriction map)", (int)nid);
    if (ntblb < 1 || ntlb < 1 || (int64_t)ntblb * ntlb > CHICDIFF_CHICAGO_MAX_PAIRS)
        return fail(c, CHICDIFF_E_INVALID, "chicago_tables: ntblb = %d, ntlb = %d (both >= 1, ntblb * ntlb <= %d: the capacity of the LDS table)",
                    (int)ntblb, (int)ntlb, CHICDIFF_CHICAGO_MAX_PAIRS);
    if (ndistbin < 0 || ndistbin > CHICDIFF_CHICAGO_MAX_DISTBIN)
        return fail(c, CHICDIFF_E_INVALID, "chicago_tables: ndistbin = %d (0 <= ndistbin <= %d: the capacity of the LDS table)", (int)ndistbin,
                    CHICDIFF_CHICAGO_MAX_DISTBIN);
    HIPCHK(c, hipSetDevice(c->device));
    if (int rc = ensure_aux(c, chicago_workspace_bytes(nid))) return rc;
    ChicagoArgs a;
    a.bait = d_bait; a.oe = d_oe; a.s_j = d_s_j; a.s_i = d_s_i; a.Tmean = d_Tmean; a.refBinMean = d_refBinMean;
    a.tblb = d_tblb; a.tlb = d_tlb; a.distbin = d_distbin; a.nrows = nrows;
    a.id_min = id_min; a.nid = nid; a.ntblb = ntblb; a.ntlb = ntlb; a.ndistbin = ndistbin;
    a.sj = d_sj; a.si = d_si; a.tblb_of = d_tblb_of; a.tlb_of = d_tlb_of; a.T = d_T; a.ref = d_ref;
    const uint32_t *d_status = nullptr;
    static const char *const stage_name[3] = {"chicago_tables_init", "chicago_tables_pass1", "chicago_tables_pass2"};
    timing_reset(c);
    for (int stage = 0; stage < 3; stage++) {
        Scope t(c, stage_name[stage]);
        launch_chicago_tables(a, stage, c->host.chicago_tables_run_merge, c->aux, c->stream, &d_status);
    }
    HIPCHK(c, hipGetLastError());
    uint32_t h = 0;
    HIPCHK(c, hipMemcpyAsync(&h, d_status, sizeof h, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    timing_collect(c);
    if (h & CHICDIFF_CHICAGO_BAD_CODE)
        return fail(c, CHICDIFF_E_INVALID, "chicago_tables: a tblb, tlb or distbin code lies outside [-1, %d) / [-1, %d) / [-1, %d)", (int)ntblb,
                    (int)ntlb, (int)ndistbin);
    *status_host = (int32_t)(h & CHICDIFF_CHICAGO_NOT_A_FUNCTION);
    return CHICDIFF_OK;
}

extern "C" int chicdiff_hip_chicago_tables_caps(int32_t *max_pairs, int32_t *max_distbin, int32_t *rows_per_workgroup) {
    if (max_pairs) *max_pairs = CHICDIFF_CHICAGO_MAX_PAIRS;
    if (max_distbin) *max_distbin = CHICDIFF_CHICAGO_MAX_DISTBIN;
    if (rows_per_workgroup) *rows_per_workgroup = CHICDIFF_CHICAGO_ROWS_PER_WORKGROUP;
    return CHICDIFF_OK;
}

// countput of one condition (chicdiff.R:708-735, 754-768): key pass, sort, heads, scan and reduce enqueued behind one another; the one
// host stop is the read of the two counts
extern "C" int chicdiff_hip_countput_dev(chicdiff_hip_ctx *c, int32_t nrep, const int32_t *const *d_bait, const int32_t *const *d_oe,
                                         const int32_t *const *d_N, const double *const *d_Bmean, const double *const *d_score,
                                         const double *const *d_distSign, const int64_t *nrows, int32_t id_min, int32_t nid,
                                         const int64_t *d_midsum, const int32_t *d_chr, int32_t *d_out_bait, int32_t *d_out_oe,
                                         double *d_Nav, double *d_Bav, double *d_out_score, double *d_mid, int64_t *ngroups_host) {
    if (!c) return CHICDIFF_E_INVALID;
    if (ngroups_host) *ngroups_host = 0;
    if (nrep < 1 || nrep > CHICDIFF_COUNTPUT_MAX_REP)
        return fail(c, CHICDIFF_E_INVALID, "countput: nrep = %d replicates (1 <= nrep <= %d: the capacity of the LDS table)", (int)nrep,
                    CHICDIFF_COUNTPUT_MAX_REP);
    if (!d_bait || !d_oe || !d_N || !d_Bmean || !d_score || !d_distSign || !nrows || !d_midsum || !d_chr || !ngroups_host)
        return fail(c, CHICDIFF_E_INVALID, "countput: bad arguments (a NULL pointer)");
    if (nid < 1) return fail(c, CHICDIFF_E_INVALID, "countput: nid = %d (an empty restriction map)", (int)nid);
    if ((int64_t)id_min + (int64_t)nid > (int64_t)INT32_MAX)
        return fail(c, CHICDIFF_E_INVALID, "countput: id_min + nid = %lld (map IDs must lie below INT32_MAX = 2147483647: the all-ones key marks "
                    "a dropped row)", (long long)id_min + (long long)nid);
    std::vector<CountputRep> reps((size_t)nrep);
    int64_t n = 0;
    for (int r = 0; r < nrep; r++) {
        if (nrows[r] < 0) return fail(c, CHICDIFF_E_INVALID, "countput: nrows[%d] = %lld (a negative number of rows)", r, (long long)nrows[r]);
        if (nrows[r] > 0 && (!d_bait[r] || !d_oe[r] || !d_N[r] || !d_Bmean[r] || !d_score[r] || !d_distSign[r]))
            return fail(c, CHICDIFF_E_INVALID, "countput: replicate %d has %lld rows and a NULL column", r, (long long)nrows[r]);
        reps[r].bait = d_bait[r]; reps[r].oe = d_oe[r]; reps[r].N = d_N[r];
        reps[r].Bmean = d_Bmean[r]; reps[r].score = d_score[r]; reps[r].distSign = d_distSign[r];
        reps[r].offset = n;
        n += nrows[r];
        if (n >= (1ll << 31))
            return fail(c, CHICDIFF_E_INVALID, "countput: the replicates hold %lld rows or more up to replicate %d (sum of nrows < 2^31: the "
                        "global row is a 32-bit sort value)", (long long)n, r);
    }
    if (n == 0) return CHICDIFF_OK;
    if (!d_out_bait || !d_out_oe || !d_Nav || !d_Bav || !d_out_score || !d_mid)
        return fail(c, CHICDIFF_E_INVALID, "countput: bad arguments (a NULL output)");
    HIPCHK(c, hipSetDevice(c->device));
    if (int rc = ensure_aux(c, countput_workspace_bytes(n))) return rc;
    CountputArgs a;
    a.nrep = nrep; a.reps = reps.data(); a.n = n; a.id_min = id_min; a.nid = nid; a.midsum = d_midsum; a.chr = d_chr;
    a.out_bait = d_out_bait; a.out_oe = d_out_oe; a.Nav = d_Nav; a.Bav = d_Bav; a.score = d_out_score; a.mid = d_mid;
    const CountputResult *d_res = nullptr;
    timing_reset(c);
    {
        Scope t(c, "countput");
        if (launch_countput(a, c->aux, c->stream, &d_res)) return fail(c, CHICDIFF_E_HIP, "countput: copy/sort/scan failed");
    }
    CountputResult h;
    HIPCHK(c, hipMemcpyAsync(&h, d_res, sizeof h, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    HIPCHK(c, hipGetLastError());
    timing_collect(c);
    *ngroups_host = (int64_t)h.ngroups;
    return CHICDIFF_OK;
}

extern "C" int chicdiff_hip_countput_caps(int32_t *max_rep, int32_t *key_rows_per_workgroup, int32_t *reduce_rows_per_workgroup) {
    if (max_rep) *max_rep = CHICDIFF_COUNTPUT_MAX_REP;
    if (key_rows_per_workgroup) *key_rows_per_workgroup = CHICDIFF_COUNTPUT_KEY_ROWS_PER_WORKGROUP;
    if (reduce_rows_per_workgroup) *reduce_rows_per_workgroup = CHICDIFF_COUNTPUT_REDUCE_ROWS_PER_WORKGROUP;
    return CHICDIFF_OK;
}

extern "C" int chicdiff_hip_count_table_dev(chicdiff_hip_ctx *c, const int32_t *d_bait, const int32_t *d_oe, const int32_t *d_N,
                                            int64_t nrows, const uint8_t *d_bait_in_RU, int32_t max_id, int64_t *d_keys,
                                            int32_t *d_vals, int64_t *nkeys_host) {
    if (!c) return CHICDIFF_E_INVALID;
    if (!d_bait || !d_oe || !d_N || !d_keys || !d_vals || !nkeys_host || nrows < 1 || nrows >= (1ll << 32) || (d_bait_in_RU && max_id < 0))
        return fail(c, CHICDIFF_E_INVALID, "count_table: bad arguments");
    HIPCHK(c, hipSetDevice(c->device));
    int rc = ensure_aux(c, ct_workspace_bytes(nrows));
    if (rc) return rc;
    timing_reset(c);
    {
        Scope t(c, "count_table");
        if (launch_count_table(d_bait, d_oe, d_N, nrows, d_bait_in_RU, max_id, d_keys, d_vals, c->aux, c->stream))
            return fail(c, CHICDIFF_E_HIP, "count_table: sort failed");
    }
    unsigned long long h = 0;
    HIPCHK(c, hipMemcpyAsync(&h, c->aux, sizeof h, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    timing_collect(c);
    *nkeys_host = (int64_t)h;
    return CHICDIFF_OK;
}

// IHWcorrection's covariate (chicdiff.R:1965-1967): per-region mean of distSign over the CSR of RU rows
extern "C" int chicdiff_hip_region_avdist_dev(chicdiff_hip_ctx *c, const int32_t *d_ru_bait, const int32_t *d_ru_oe, int64_t nru,
                                              const int64_t *d_region_ptr, int64_t n, int32_t id_min, int32_t nid,
                                              const int64_t *d_midsum, const int32_t *d_chr, double *d_avDist) {
    if (!c) return CHICDIFF_E_INVALID;
    if (!d_region_ptr || !d_midsum || !d_avDist || n < 1 || nru < 0 || nid < 1 || (nru > 0 && (!d_ru_bait || !d_ru_oe)))
        return fail(c, CHICDIFF_E_INVALID, "region_avdist: bad arguments");
    HIPCHK(c, hipSetDevice(c->device));
    timing_reset(c);
    {
        Scope t(c, "region_avdist");
        launch_region_avdist(d_ru_bait, d_ru_oe, d_region_ptr, n, id_min, nid, d_midsum, d_chr, d_avDist, c->stream);
    }
    HIPCHK(c, hipStreamSynchronize(c->stream));
    timing_collect(c);
    return CHICDIFF_OK;
}

// a1 for all replicates in one pass (chicdiff.R:843-858, the loop over the replicates): out = S x nru, column s = merge(RU, table s, all.x = TRUE)
extern "C" int chicdiff_hip_count_join_multi_dev(chicdiff_hip_ctx *c, const int32_t *d_ru_bait, const int32_t *d_ru_oe, int64_t nru,
                                                 int32_t S, const int64_t *const *d_keys, const int32_t *const *d_vals,
                                                 const int64_t *nkeys, int32_t *d_out) {
    if (!c) return CHICDIFF_E_INVALID;
    if (!d_ru_bait || !d_ru_oe || !d_out || !d_keys || !d_vals || !nkeys || nru < 0 || S < 1 || S > kMaxS)
        return fail(c, CHICDIFF_E_INVALID, "count_join_multi: bad arguments");
    for (int s = 0; s < S; s++)
        if (nkeys[s] < 0 || (nkeys[s] > 0 && (!d_keys[s] || !d_vals[s])))
            return fail(c, CHICDIFF_E_INVALID, "count_join_multi: bad table %d", s);
    HIPCHK(c, hipSetDevice(c->device));
    timing_reset(c);
    if (nru > 0) {
        if (int rc = ensure_aux(c, count_join_multi_scratch_bytes(S, nkeys))) return rc;
        Scope t(c, "count_join_multi");
        launch_count_join_multi(d_ru_bait, d_ru_oe, nru, S, d_keys, d_vals, nkeys, d_out, c->aux, c->stream);
    }
    HIPCHK(c, hipStreamSynchronize(c->stream));
    timing_collect(c);
    return CHICDIFF_OK;
}

// a1 + a3 + a2 fused (chicdiff.R:843-858, 628-703, 894-896, 1540-1547; chinput branch): region-level N and FullMean without the two
// per-fragment matrices — bit for bit count_join_multi -> fragment_background -> window_sums
extern "C" int chicdiff_hip_region_assemble_dev(chicdiff_hip_ctx *c, const int32_t *d_ru_bait, const int32_t *d_ru_oe, int64_t nru,
                                                const int64_t *d_region_ptr, int64_t n, int32_t S, const int64_t *const *d_keys,
                                                const int32_t *const *d_vals, const int64_t *nkeys, int32_t id_min, int32_t nid,
                                                const int64_t *d_midsum, const double *d_sj, const double *d_si, const int32_t *d_tblb,
                                                const int32_t *d_tlb, const double *d_T, int32_t ntblb, int32_t ntlb,
                                                const double *distfun_host, int32_t *d_N, double *d_FullMean) {
    if (!c) return CHICDIFF_E_INVALID;
    if (S < 1 || S > kMaxS) return fail(c, CHICDIFF_E_INVALID, "region_assemble: need 1 <= S <= %d (S = %d)", kMaxS, (int)S);
    if (!d_region_ptr || n < 1 || nru < 0 || (nru > 0 && (!d_ru_bait || !d_ru_oe)))
        return fail(c, CHICDIFF_E_INVALID, "region_assemble: bad arguments (region_ptr / n / nru / RU rows)");
    if (!d_N && !d_FullMean) return fail(c, CHICDIFF_E_INVALID, "region_assemble: neither N nor FullMean is asked for");
    if (d_N) {
        if (!d_keys || !d_vals || !nkeys) return fail(c, CHICDIFF_E_INVALID, "region_assemble: N needs the key tables");
        for (int s = 0; s < S; s++)
            if (nkeys[s] < 0 || (nkeys[s] > 0 && (!d_keys[s] || !d_vals[s])))
                return fail(c, CHICDIFF_E_INVALID, "region_assemble: bad table %d", s);
    }
    if (d_FullMean && (!d_midsum || !d_sj || !d_si || !d_tblb || !d_tlb || !d_T || !distfun_host || nid < 1 || ntblb < 1 || ntlb < 1))
        return fail(c, CHICDIFF_E_INVALID, "region_assemble: FullMean needs the background tables");
    HIPCHK(c, hipSetDevice(c->device));
    // the context's scratch: the distance functions, then the coarse levels of the key tables
    const size_t df_bytes = sizeof(double) * 10 * kMaxS;
    if (int rc = ensure_aux(c, df_bytes + (d_N ? count_join_multi_scratch_bytes(S, nkeys) : 0))) return rc;
    double *d_df = reinterpret_cast<double *>(c->aux);
    hipError_t e = hipSuccess;
    if (d_FullMean) e = hipMemcpyAsync(d_df, distfun_host, sizeof(double) * 10 * S, hipMemcpyHostToDevice, c->stream);
    timing_reset(c);
    hipError_t le = hipSuccess;
    if (e == hipSuccess) {
        Scope t(c, "region_assemble");
        le = launch_region_assemble(d_ru_bait, d_ru_oe, nru, d_region_ptr, n, S, d_keys, d_vals, nkeys, id_min, nid, d_midsum, d_sj, d_si,
                                    d_tblb, d_tlb, d_T, ntblb, ntlb, d_df, d_N, d_FullMean, c->aux + df_bytes, c->host.region_assemble_generic,
                                    c->stream);
    }
    if (e == hipSuccess) e = hipStreamSynchronize(c->stream);  // distfun_host may be a temporary
    timing_collect(c);
    if (le != hipSuccess) return fail(c, CHICDIFF_E_HIP, "region_assemble: launch of region_assemble_kernel failed: %s", hipGetErrorString(le));
    if (e != hipSuccess) return fail(c, CHICDIFF_E_HIP, "region_assemble: %s", hipGetErrorString(e));
    return CHICDIFF_OK;
}

// a1 without chinput files (chicdiff.R:774-807): N of every RU row from the replicates' Chicago tables, inner-merged
extern "C" int chicdiff_hip_count_join_inner_dev(chicdiff_hip_ctx *c, const int32_t *d_ru_bait, const int32_t *d_ru_oe, int64_t nru,
                                                 int32_t S, const int64_t *const *d_keys, const int32_t *const *d_vals,
                                                 const int64_t *nkeys, int32_t *d_out) {
    if (!c) return CHICDIFF_E_INVALID;
    if (!d_ru_bait || !d_ru_oe || !d_out || !d_keys || !d_vals || !nkeys || nru < 0 || S < 1 || S > kMaxS)
        return fail(c, CHICDIFF_E_INVALID, "count_join_inner: bad arguments");
    for (int s = 0; s < S; s++)
        if (nkeys[s] < 0 || (nkeys[s] > 0 && (!d_keys[s] || !d_vals[s])))
            return fail(c, CHICDIFF_E_INVALID, "count_join_inner: bad table %d", s);
    HIPCHK(c, hipSetDevice(c->device));
    timing_reset(c);
    if (nru > 0) {
        Scope t(c, "count_join_inner");
        launch_count_join_inner(d_ru_bait, d_ru_oe, nru, S, d_keys, d_vals, nkeys, d_out, c->stream);
    }
    HIPCHK(c, hipStreamSynchronize(c->stream));
    timing_collect(c);
    return CHICDIFF_OK;
}

// a1 without chinput files, the merge alone (chicdiff.R:778, the Reduce(merge) of :774-807 and :1202-1260): the pairs every replicate
// holds, each with its S counts.  count_join_multi / region_assemble on the merged tables equal count_join_inner on the original ones.
extern "C" int chicdiff_hip_count_tables_merge_dev(chicdiff_hip_ctx *c, int32_t S, const int64_t *const *d_keys, const int32_t *const *d_vals,
                                                   const int64_t *nkeys, int64_t cap, int64_t *d_keys_out, int32_t *d_vals_out,
                                                   int64_t *n_out) {
    if (!c) return CHICDIFF_E_INVALID;
    if (S < 1 || S > kMaxS) return fail(c, CHICDIFF_E_INVALID, "count_tables_merge: need 1 <= S <= %d (S = %d)", kMaxS, (int)S);
    if (!d_keys || !d_vals || !nkeys || !n_out || cap < 0) return fail(c, CHICDIFF_E_INVALID, "count_tables_merge: bad arguments (a NULL pointer)");
    int64_t np = INT64_MAX;
    for (int s = 0; s < S; s++) {
        if (nkeys[s] < 0 || (nkeys[s] > 0 && (!d_keys[s] || !d_vals[s]))) return fail(c, CHICDIFF_E_INVALID, "count_tables_merge: bad table %d", s);
        np = nkeys[s] < np ? nkeys[s] : np;
    }
    if (cap < np)
        return fail(c, CHICDIFF_E_INVALID, "count_tables_merge: room for %lld rows needed (the smallest table), %lld given (nothing was written)",
                    (long long)np, (long long)cap);
    if (np > 0 && (!d_keys_out || !d_vals_out)) return fail(c, CHICDIFF_E_INVALID, "count_tables_merge: bad arguments (a NULL output)");
    HIPCHK(c, hipSetDevice(c->device));
    timing_reset(c);
    *n_out = 0;
    if (np == 0) return CHICDIFF_OK;  // an empty table: no pair is held by all
    const size_t ws_bytes = (count_merge_scratch_bytes(S, nkeys) + 255) / 256 * 256;
    const int64_t ntile_max = (np + 511) / 512;
    const size_t scan_bytes = ru_scan_bytes(ntile_max);
    if (int rc = ensure_aux(c, ws_bytes + scan_bytes)) return rc;
    int64_t *start = nullptr, ntile = 0;
    hipError_t le = hipSuccess;
    int sc = 0;
    {
        Scope t(c, "count_merge_mark");
        le = launch_count_merge(0, S, d_keys, d_vals, nkeys, cap, d_keys_out, d_vals_out, c->aux, &start, &ntile, c->stream);
    }
    if (le == hipSuccess) {
        Scope t(c, "count_merge_scan");
        sc = launch_scan_i64(start, ntile, c->aux + ws_bytes, scan_bytes, c->stream);
    }
    if (le == hipSuccess && sc == 0) {
        Scope t(c, "count_merge_write");
        le = launch_count_merge(1, S, d_keys, d_vals, nkeys, cap, d_keys_out, d_vals_out, c->aux, &start, &ntile, c->stream);
    }
    long long h = 0;
    hipError_t e = hipSuccess;
    if (le == hipSuccess && sc == 0) e = hipMemcpyAsync(&h, start + ntile, sizeof h, hipMemcpyDeviceToHost, c->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(c->stream);
    timing_collect(c);
    if (le != hipSuccess) return fail(c, CHICDIFF_E_HIP, "count_tables_merge: a launch failed: %s", hipGetErrorString(le));
    if (sc) return fail(c, CHICDIFF_E_HIP, "count_tables_merge: scan failed");
    if (e != hipSuccess) return fail(c, CHICDIFF_E_HIP, "count_tables_merge: %s", hipGetErrorString(e));
    *n_out = (int64_t)h;
    return CHICDIFF_OK;
}

// ---- a9: results() on device -----------------------------------------------------------------------------------
extern "C" int chicdiff_hip_cooks_filter_dev(chicdiff_hip_ctx *c, const int32_t *d_counts, int64_t n, int32_t S, const int32_t *group,
                                             const double *d_maxCooks, const int32_t *d_cooksArgmax, double cutoff, double *d_pvalue,
                                             int64_t *n_outliers_host) {
    if (!c) return CHICDIFF_E_INVALID;
    if (!d_counts || !d_maxCooks || !d_cooksArgmax || !d_pvalue || !n_outliers_host) return fail(c, CHICDIFF_E_INVALID, "cooks_filter: NULL pointer");
    FitDims d;
    int rc = check_counts_group(c, n, S, group, d);
    if (rc) return rc;
    HIPCHK(c, hipSetDevice(c->device));
    if ((rc = ensure_aux(c, 256))) return rc;
    timing_reset(c);
    {
        Scope t(c, "cooks_filter");
        launch_cooks_filter(d_counts, n, S, d.p, d_maxCooks, d_cooksArgmax, cutoff, d_pvalue, (unsigned long long *)c->aux, c->stream);
    }
    unsigned long long h = 0;
    HIPCHK(c, hipMemcpyAsync(&h, c->aux, sizeof h, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    timing_collect(c);
    *n_outliers_host = (int64_t)h;
    return CHICDIFF_OK;
}

extern "C" int chicdiff_hip_independent_filtering_dev(chicdiff_hip_ctx *c, const double *d_baseMean, const double *d_pvalue, int64_t n,
                                                      double alpha, double *d_padj, chicdiff_results_info *info) {
    if (!c) return CHICDIFF_E_INVALID;
    if (!d_baseMean || !d_pvalue || !d_padj || !info || n < 1 || n >= (1ll << 32) || !(alpha > 0 && alpha < 1))
        return fail(c, CHICDIFF_E_INVALID, "independent_filtering: bad arguments");
    HIPCHK(c, hipSetDevice(c->device));
    int rc = ensure_aux(c, if_workspace_bytes(n));
    if (rc) return rc;
    if (!c->copy_stream) HIPCHK(c, hipStreamCreateWithFlags(&c->copy_stream, hipStreamNonBlocking));
    if (!c->ev_fork) HIPCHK(c, hipEventCreateWithFlags(&c->ev_fork, hipEventDisableTiming));
    if (!c->ev_join) HIPCHK(c, hipEventCreateWithFlags(&c->ev_join, hipEventDisableTiming));
    timing_reset(c);
    {
        Scope t(c, "independent_filtering");
        const int rf = run_independent_filtering(d_baseMean, d_pvalue, n, alpha, d_padj, c->aux, c->stream, c->copy_stream, c->ev_fork, c->ev_join, info);
        if (rf == 2) return fail(c, CHICDIFF_E_INVALID, "independent_filtering: NaN baseMean (quantile() stops on missing values)");
        if (rf) return fail(c, CHICDIFF_E_HIP, "independent_filtering: %s", hipGetErrorString(hipGetLastError()));
    }
    HIPCHK(c, hipStreamSynchronize(c->stream));
    timing_collect(c);
    return CHICDIFF_OK;
}
