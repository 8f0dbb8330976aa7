/*
 * chicdiff_hip.h — C ABI of the MI355X-native differential-testing core of Chicdiff.
 *
 * The reference (pure R, /root/reference/Chicdiff/R/chicdiff.R) has no FFI: the seam it
 * offers is the exported R function DESeq2Wrap() (chicdiff.R:1494) and, below it, the DESeq2
 * calls at chicdiff.R:1557-1674.  Each entry point here replaces one of those call groups and
 * is what an R `.Call` shim (r/src/chicdiff_hip_shim.c) binds.  No R, no
 * torch, no C++ types cross this boundary: plain pointers, sizes and a status code.
 *
 * Conventions
 *   - matrices are n x S column-major (= sample-major; element (i, j) at [j*n + i]): exactly
 *     R's INTEGER(mat)/REAL(mat) for the matrices built at chicdiff.R:1551-1553 and :1583,
 *     and the coalesced layout for one-row-per-lane kernels.
 *   - `_dev` entry points take DEVICE pointers (HBM-resident inputs/outputs, the benchmarked
 *     form); the others take caller-owned HOST buffers and stage them (what R passes).
 *   - every function returns 0 on success, a CHICDIFF_E_* code otherwise;
 *     chicdiff_hip_last_error() gives the message.  Nothing throws, aborts or calls exit.
 *   - NA: counts must not be NA_integer_ (INT_MIN) -> CHICDIFF_E_INVALID; NaN/NA_real_ in
 *     FullMean is meaningful (row falls back to size factors, chicdiff.R:1588-1589).
 *   - threading: call from one host thread per context; work is enqueued on the context's
 *     stream (chicdiff_hip_set_stream) and the call returns after the results are complete.
 */
#ifndef CHICDIFF_HIP_H
#define CHICDIFF_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define CHICDIFF_OK 0
#define CHICDIFF_E_INVALID 1   /* bad argument (shape, NA count, unsupported design)          */
#define CHICDIFF_E_HIP 2       /* HIP runtime error (message has hipGetErrorString)           */
#define CHICDIFF_E_NOMEM 3
#define CHICDIFF_E_COMM 4      /* all-reduce callback failed                                  */
#define CHICDIFF_E_NUMERIC 5   /* e.g. every row has a zero (size factors undefined)          */

/* status bits reported in chicdiff_nbglm_scalars.status (fit completed, with caveats) */
#define CHICDIFF_ST_TREND_FAILED 1 /* no dispersion trend: the parametric fit failed and so did its substitute, the local regression
                                      (fewer than four usable rows), or the substitution was switched off (option
                                      local_trend_substitute = 0) — refit with opts.fitType = 1 ("mean") or supply trendCoef */
#define CHICDIFF_ST_PRIORVAR_MC 2  /* m-p<=3 and no dispPriorVar given: matched by simulation as DESeq2 does it (its set.seed(2) stream, hist(), loess()) */
#define CHICDIFF_ST_BETA_NONCONV 4 /* some rows hit betaMaxit (DESeq2 would call optim)        */
#define CHICDIFF_ST_ALLZERO_ROWS 8 /* some rows are all zero: their outputs are NaN (R: NA)    */
#define CHICDIFF_ST_TREND_LOCAL 16 /* dispFit is DESeq2's local-regression trend (localDispersionFit = locfit with its defaults): asked for
                                      (fitType 2), or substituted for a failed parametric fit as estimateDispersionsFit does;
                                      trendCoef is NaN */

typedef struct chicdiff_hip_ctx chicdiff_hip_ctx;

/* Sum-all-reduce `count` doubles at DEVICE pointer `dev_buf`, in place, ordered on the
 * context's stream, across the ranks sharing the fit.  Return 0 on success.  Replaces nothing
 * in the reference (single process); it is the hook for row sharding. */
typedef int (*chicdiff_allreduce_fn)(void *user, void *dev_buf, int64_t count);

/* Optional companion of the all-reduce hook: every rank contributes `count` doubles at DEVICE pointer `dev_send`; `dev_recv`
 * (world_size x count doubles, distinct from dev_send) receives rank r's block at r * count, ordered on the context's stream.
 * With it a sharded fit exchanges the rows of the dispersion trend by one all-gather (ncclAllGather); without it, by a
 * sum-all-reduce over zero-filled all-ranks arrays (twice the bytes).  Same results either way. */
typedef int (*chicdiff_allgather_fn)(void *user, const void *dev_send, void *dev_recv, int64_t count);

int chicdiff_hip_create(chicdiff_hip_ctx **ctx, int32_t device);
void chicdiff_hip_destroy(chicdiff_hip_ctx *ctx);
const char *chicdiff_hip_last_error(const chicdiff_hip_ctx *ctx); /* ctx may be NULL: last create() error */
/* hipStream_t to enqueue on (NULL = HIP's null stream).  Until this is called the context
 * uses a private non-blocking stream. */
int chicdiff_hip_set_stream(chicdiff_hip_ctx *ctx, void *hip_stream);
/* A non-NULL callback turns every global statistic (size-factor medians, nf column means, trend
 * sums, MAD medians, deviance sums) into local partials + one callback (also with world_size 1,
 * where the all-reduce is the identity); fn = NULL restores the single-process path. */
int chicdiff_hip_set_allreduce(chicdiff_hip_ctx *ctx, chicdiff_allreduce_fn fn, void *user,
                               int32_t world_size, int32_t rank);
/* After chicdiff_hip_set_allreduce (which clears it): the all-gather of the same transport; fn = NULL removes it. */
int chicdiff_hip_set_allgather(chicdiff_hip_ctx *ctx, chicdiff_allgather_fn fn, void *user);
/* Refits the last fit / size-factor / Wald-test call went through (a sharded select whose candidate list overflowed on some
 * rank, a grid-barrier timeout of the trend kernel on some rank, the local-regression substitute): every rank of a sharded
 * call reports the same number — each verdict is all-reduced before anybody acts on it. */
int32_t chicdiff_hip_last_refits(const chicdiff_hip_ctx *ctx);

/* Tuning / test options; the defaults are what bench.py measures.  (Every option the library accepts, in the order of its
 * table — kOptions in chicdiff_amd/csrc/ctx.hip; any other name or value is CHICDIFF_E_INVALID.)
 * Results and options: five options select another summation order and so move results at the 1e-13 level (about one row in
 * 1e5 then stops a line search one step apart) — "trend_one_launch_per_pass" and "sharded_trend_gather"
 * (the trend's sums over another partition of the rows), "theta_grid_concurrency" through the route of its lanes (more than one
 * fit in flight: every fit of the grid has its trend as one launch per pass, and is the single fit under
 * "trend_one_launch_per_pass" = 1 bit for bit, whatever the number of lanes; one fit in flight or a one-point grid: the default
 * single fit, bit for bit), "trend_persistent_blocks" (the partition of the single-launch trend kernel) and
 * "wald_final_row_constant" (`deviance` and `sumDeviance` alone).  Every other option is bit-neutral ("same bits" below), but for
 * "local_trend_substitute" at the end of the list.  tests/test_gpu_theta_scan.py holds the lanes' route to the 50-digit twin and
 * the grid to the single fits.
 *   "line_search_spread"        1 (default) | 0 | 2 | 3: evaluate straggler rows (line searches and IRLS) with their samples spread across
 *                               lanes; 0 = row per lane only; 2 = as 1 without the lean tick of the launch's end, 3 = as 1 without the layouts of
 *                               more than 128 exchange entries (bit-identity tests)
 *   "line_search_min_waves"     0 (default: by the launcher's rule) | 2 .. 4: waves per SIMD the line-search kernel variant is built for
 *   "line_search_chunk"         0 (default: chosen from the row count) | 8 .. 64: rows per dequeue of the line searches
 *   "line_search_prio"          0 (default: off) .. 100: line-search waves raise their issue priority with the age of their search, one
 *                               level per this many iterations
 *   "line_search_schedule"      1 (default) | 0 | 3 | 4: the gene-wise line search visits the rows likely to need DESeq2's full 100
 *                               iterations first (score alpha_init * smaller group mean, in classes of 1/8 decade; the rows that
 *                               start at minDisp in front of the score >= 3.16 rows); 0 = natural row order; 3 = the six
 *                               half-decade classes of earlier releases (minDisp starts last); 4 = as 1, minDisp starts last
 *                               (2 is not a mode)
 *   "line_search_deal"          0 (default: chosen from the rows per wave), 1 .. 64: schedule entries per group of the static deal
 *   "line_search_classes_a"     0 (default: by the launcher's rule) | 1 .. 6: half-decade score classes of the schedule that are dealt
 *                               out to the waves statically instead of going through the queue
 *   "line_search_fillers"       -1 (default: by the launcher's rule) | 0 | 1: the gene-wise line search runs its two waves per SIMD at
 *                               issue priority and adds a third at priority 0 that takes only rows from the schedule's end (score >= 3.16:
 *                               never long); always off where the schedule has no class order ("line_search_schedule" 0, small fits)
 *                               and at S > 8
 *   "line_search_filler_stop"   -1 (default: 85) | 0 .. 100: fillers stop claiming once the other waves have claimed this share (percent) of
 *                               their own part of the queue (100 = never, 0 = fillers claim nothing)
 *   "theta_grid_concurrency"    5 (default), 1 .. 16: fits of the theta grid in flight at once (single rank only)
 *   "host_copy_threads"         12 (default), 1 .. 64: host threads staging caller buffers in chicdiff_hip_nbglm_fit
 *   "select_all_rounds"         0 (default) | 1: exact medians by histogram rounds only (no candidate-sort shortcut; the size factors of a
 *                               single-rank call with S <= 16: by the radix select over stored keys instead of two passes over the counts)
 *   "trend_one_launch_per_pass" 0 (default) | 1: trend fit as one launch per IRLS pass instead of one persistent kernel
 *   "sharded_trend_gather"      1 (default) | 0: sharded fits exchange the trend's rows once and fit them on every rank,
 *                               instead of one all-reduce per IRLS pass (same coefficients up to summation order)
 *   "trend_persistent_blocks"   0 (default: one workgroup per CU), 1 .. 256: cap on the workgroups of the single-launch trend
 *                               kernel, for fits that share one GPU (its grid barrier needs all of them resident at once); the
 *                               coefficients then differ in summation order only (1e-13)
 *   "trend_speculate"           1 (default) | 0: passes of the single-launch trend kernel that are likely to end a glm() call also sum
 *                               what the next call's start pass would, so that pass is not run; 0 = every pass is run: same bits
 *   "trend_exchange"            1 (default) | 0: the workgroups of the single-launch trend kernel hand each other a pass's partial sums as
 *                               64-bit words that carry the pass number beside half a double, polled without fences; 0 = every pass
 *                               publishes its sums, crosses a grid barrier and reads them back: same bits
 *   "mad_select_route"          1 (default) | 0: the single-launch trend kernel takes the median and MAD of the residuals from one histogram over
 *                               their values (three grid-wide rounds, radix select only where a candidate list does not fit); 0 = two
 *                               radix selects (six rounds): same bits
 *   "mad_value_cap"             0 (default: 8000) | 1 .. 8000: test hook, keys a candidate list of that histogram route may hold
 *   "trend_mad_in_kernel"       1 (default) | 0: the single-launch trend kernel goes on to the residuals, their exact median and MAD
 *                               and the closed-form prior variance; 0 = separate launches (residuals, two radix selects): same bits
 *   "fuse_offsets"              1 (default) | 0 | 2: chicdiff_hip_wald_test_dev and the theta grid form the offsets inside the fit's
 *                               first kernel wherever that was measured to be the faster route — since the kernels are built by
 *                               sample class that is every fit at S <= 16; 0 = always by a launch of their own, 2 = always inside
 *                               (at S <= 16): same bits
 *   "prep_blocks"               0 (default: one resident round, sized by the runtime's occupancy query) | 1 .. 1024: test handle, at
 *                               most this many workgroups for the fit's first kernel at S <= 16, so that a fit of a few thousand
 *                               rows runs several tiles per workgroup: same bits
 *   "region_assemble_generic"   0 (default) | 1: test option of chicdiff_hip_region_assemble_dev (see there): same bits
 *   "chicago_tables_run_merge"  1 (default) | 0: chicdiff_hip_chicago_tables_dev merges runs of rows that aim at one fragment's slot inside the
 *                               wave before the global atomic (tables keyed by bait); 0 = one atomic per row: same bits
 *   "table_write_half_kib"      0 (default: 64 MiB at most) | 4 .. 65536: test handle, KiB of one half of the pinned area that
 *                               chicdiff_hip_table_write_dev moves the text through (small values make a small table take many halves)
 *   "fault_inject"              0 (default) .. 7; test hook, one-shot bits consumed by the next call: 1 = this rank reports a select
 *                               overflow in its next fit, 2 = a grid-barrier timeout of its trend kernel, 4 = an overflow of its
 *                               next size-factor select — to prove that all ranks of a sharded fit refit together
 *   "bench_fake_world"          0 (default) | 1 .. 64: rehearsal hook of bench.py, refused above 1 unless CHICDIFF_BENCH_FAKE_WORLD is set
 *                               in the environment: on a 1-rank communicator the trend's rows are gathered as if this many ranks had
 *                               each sent this rank's block (a rank's step of an N-GPU fit at its share of the rows)
 *   "sf_log_table"              1 (default) | 0: the two passes of the single-rank size-factor route (S <= 16) take the logarithm of a
 *                               count below 2048 from a table each workgroup fills in LDS with the very function it replaces;
 *                               0 = a table-driven logarithm per count: same bits
 *   "wald_final_row_constant"   1 (default) | 0: the Wald stage's last kernel takes sum_j y_j log(alpha mu_j) of a row the IRLS
 *                               converged on from the row constant and the group sums of the counts instead of a logarithm per
 *                               sample: `deviance` and `sumDeviance` differ in summation order only (1e-13), every other output
 *                               has the same bits
 * and one that does change the outcome of a fit whose parametric trend fails (DESeq2 offers the same choice through fitType):
 *   "local_trend_substitute"    1 (default) | 0: report CHICDIFF_ST_TREND_FAILED instead of substituting the local regression */
int chicdiff_hip_set_option(chicdiff_hip_ctx *ctx, const char *name, int64_t value);

/* Direct RCCL (backend of choice on one node: RCCL over xGMI).  The library dlopen()s librccl (librccl_path, or
 * "librccl.so" when NULL/empty — pass the copy the host process already uses, e.g. torch's), creates its own
 * communicator and from then on calls ncclAllReduce(ncclFloat64, ncclSum) — and ncclAllGather for the rows of the
 * dispersion trend — itself, in place on its stream: no host callback per collective.  Rank 0 makes the 128-byte id with _unique_id and the host broadcasts it (any
 * transport); every rank then calls _init, which replaces a callback set with chicdiff_hip_set_allreduce. */
int chicdiff_hip_rccl_unique_id(chicdiff_hip_ctx *ctx, const char *librccl_path, void *id128);
int chicdiff_hip_rccl_init(chicdiff_hip_ctx *ctx, const char *librccl_path, const void *id128, int32_t world_size,
                           int32_t rank);

/* Device memory for hosts without a GPU array library of their own (the R shim): plain allocations on the
 * context's device, copies ordered on the context's stream and complete on return.  The context keeps a list of
 * them: chicdiff_hip_destroy() releases whatever is still outstanding (R runs the finalizers of one garbage
 * collection in no particular order, so a context can be finalized before its vectors — r/src/chicdiff_hip_shim.c:
 * devbuf_finalizer then finds the context gone and has nothing left to free); chicdiff_hip_free() of a pointer the
 * context does not own is CHICDIFF_E_INVALID.  _outstanding_allocations: how many are live (-1: NULL context). */
int chicdiff_hip_malloc(chicdiff_hip_ctx *ctx, uint64_t bytes, void **d_ptr);
int chicdiff_hip_free(chicdiff_hip_ctx *ctx, void *d_ptr);
int64_t chicdiff_hip_outstanding_allocations(chicdiff_hip_ctx *ctx);
int chicdiff_hip_memcpy_h2d(chicdiff_hip_ctx *ctx, void *d_dst, const void *h_src, uint64_t bytes);
int chicdiff_hip_memcpy_d2h(chicdiff_hip_ctx *ctx, void *h_dst, const void *d_src, uint64_t bytes);

/* DESeq2 defaults that Chicdiff never overrides (chicdiff.R:1573-1574 pass no arguments). */
typedef struct {
    double minDisp;      /* 1e-8 */
    double dispTol;      /* 1e-6 */
    double kappa0;       /* 1.0  */
    int32_t maxit;       /* 100  dispersion line search */
    int32_t betaMaxit;   /* 100  Wald IRLS              */
    double betaTol;      /* 1e-8 */
    double minmu;        /* 0.5  */
    double outlierSD;    /* 2.0  */
    double dispPriorVar; /* NaN = estimate; DESeq2's estimateDispersionsMAP(dispPriorVar=) */
    double trendCoef[2]; /* NaN = fit; else use alpha(mu) = c0 + c1/mu as given (DESeq2: dispersionFunction<-) */
    int32_t fitType;     /* 0 = "parametric" (DESeq2's and Chicdiff's default; when that fit fails the local regression is
                            substituted, as DESeq2 does, and CHICDIFF_ST_TREND_LOCAL is set);
                            1 = "mean": dispFit = mean(dispGeneEst[dispGeneEst > 10 minDisp], trim = 0.001) for every row,
                            DESeq2's estimateDispersions(fitType = "mean") (single process only);
                            2 = "local": locfit(log dispGeneEst ~ log baseMean, weights = baseMean) with locfit's defaults */
    int32_t _pad;
} chicdiff_nbglm_opts;
void chicdiff_hip_default_opts(chicdiff_nbglm_opts *opts);

/* Per-row outputs, length n each; any pointer may be NULL (not wanted).  Host or device
 * pointers according to the entry point used.  The device entry points write these columns IN PLACE while the fit
 * runs (its workspace points into them), so after a return other than CHICDIFF_OK — and while a fit that had to
 * start over is under way — their contents are undefined: partly written, not "untouched". */
typedef struct {
    double *baseMean;       /* mcols(dds)$baseMean                                   */
    double *baseVar;
    double *dispGeneEst;    /* mcols(dds)$dispGeneEst                                */
    double *dispFit;        /* mcols(dds)$dispFit                                    */
    double *dispMAP;
    double *dispersion;     /* dispersions(dds)                                      */
    double *log2FoldChange; /* results(dds)$log2FoldChange (NaN for design ~1)       */
    double *lfcSE;
    double *stat;
    double *pvalue;         /* before Cook's cutoff / independent filtering          */
    double *intercept;      /* log2 scale                                            */
    double *interceptSE;
    double *deviance;       /* mcols(dds)$deviance = -2 logLik                       */
    double *maxCooks;       /* NaN unless a group has >= 3 samples                   */
    int32_t *dispGeneIter, *dispIter, *dispOutlier, *betaConv, *betaIter, *allZero;
    int32_t *cooksArgmax;   /* 0-based sample with the largest Cook's distance (-1 if none)   */
} chicdiff_nbglm_out;

typedef struct {
    double trendCoef[2];    /* asymptDisp, extraPois: attr(dispersionFunction, "coefficients") */
    double varLogDispEsts;
    double dispPriorVar;
    double sumDeviance;     /* sum(mcols(dds)$deviance) as chicdiff.R:1647 (NaN if any all-zero row) */
    int64_t nAllZero;
    int32_t trendOuterIter;
    int32_t status;         /* CHICDIFF_ST_* bits */
} chicdiff_nbglm_scalars;

/* a5 — estimateSizeFactors (chicdiff.R:1561-1562): median-of-ratios, S doubles to HOST sf. */
int chicdiff_hip_size_factors_dev(chicdiff_hip_ctx *ctx, const int32_t *d_counts, int64_t n, int32_t S,
                                  double *sf_host);

/* a4 — offsets (chicdiff.R:1583-1589 M3; :1614-1615 nsf; :1635-1638 / :1666-1669 theta mix).
 * theta = NaN returns normFactorsM3 (norm="fullmean"); otherwise sc(theta).  d_fullMean = NULL returns the size
 * factors, one column per sample (norm="standard", chicdiff.R:1572-1575). */
int chicdiff_hip_offsets_dev(chicdiff_hip_ctx *ctx, const double *d_fullMean, const double *sf_host,
                             int64_t n, int32_t S, double theta, double *d_nf_out);

/* a2 — window sums (chicdiff.R:1540-1556).  Fragments of region i are rows
 * [region_ptr[i], region_ptr[i+1]) of the nfrag x S fragment matrices (ascending otherEndID,
 * the order setkey(fragData, otherEndID) at :1526 produces).  Either input may be NULL. */
int chicdiff_hip_window_sums_dev(chicdiff_hip_ctx *ctx, const int32_t *d_fragN, const double *d_fragFullMean,
                                 int64_t nfrag, int32_t S, const int64_t *d_region_ptr, int64_t n,
                                 int32_t *d_N, double *d_FullMean);

/* a1 — count join (chicdiff.R:843-858): out[r] = N of (bait[r], oe[r]) in the sample's sorted
 * key table (key = baitID<<32 | otherEndID, ascending, unique), 0 when absent. */
int chicdiff_hip_count_join_dev(chicdiff_hip_ctx *ctx, const int32_t *d_ru_bait, const int32_t *d_ru_oe,
                                int64_t nru, const int64_t *d_keys, const int32_t *d_vals, int64_t nkeys,
                                int32_t *d_out);

/* a1 for ALL replicates in one pass (chicdiff.R:843-858: the loop `for (i in 1:length(chicdiff.settings$countData))` around
 * merge(RU, temp, all.x = TRUE)): every replicate's column of N from one read of the RU rows.  d_keys / d_vals / nkeys are HOST
 * arrays of S entries (device pointers inside), one sorted key table per replicate; d_out is nru x S column-major (column s =
 * replicate s) and equals S calls of chicdiff_hip_count_join_dev bit for bit. */
int chicdiff_hip_count_join_multi_dev(chicdiff_hip_ctx *ctx, const int32_t *d_ru_bait, const int32_t *d_ru_oe, int64_t nru,
                                      int32_t S, const int64_t *const *d_keys, const int32_t *const *d_vals,
                                      const int64_t *nkeys, int32_t *d_out);

/* a1 + a3 + a2 in one kernel, chinput branch (chicdiff.R:843-858 the joins, :628-703 and :894-896 FullMean = Bmean + Tmean,
 * :1540-1547 the per-region sums): region-level N and FullMean straight from the RU rows, the replicates' key tables and the
 * Chicago background tables.  Nothing of size S x nru is allocated or written.
 * CONTRACT: equal, bit for bit, to chicdiff_hip_count_join_multi_dev -> chicdiff_hip_fragment_background_dev (FullMean) ->
 * chicdiff_hip_window_sums_dev on the same arguments, which stay for callers who want per-fragment values.
 * d_ru_bait / d_ru_oe / nru, d_keys / d_vals / nkeys (HOST arrays of S entries, device pointers inside): as in
 * chicdiff_hip_count_join_multi_dev; d_region_ptr / n: as in chicdiff_hip_window_sums_dev (an empty region gives 0 / 0.0; rows
 * outside [0, nru) are never read); id_min .. distfun_host (S x 10, host): as in chicdiff_hip_fragment_background_dev.
 * d_N (int32) and d_FullMean (double) are n x S column-major (column s = replicate s); either may be NULL, and then the key
 * tables respectively the background tables are not read and may be NULL too.  1 <= S <= 64.
 * The branch without chinput files (a pair counts only where every replicate holds it) is served through
 * chicdiff_hip_count_tables_merge_dev: this call on the merged tables equals chicdiff_hip_count_join_inner_dev and the two
 * calls after it on the original ones.
 * Test option "region_assemble_generic" (chicdiff_hip_set_option) 0 (default) | 1: every tile of regions takes the kernel's
 * generic path (one region per lane, a search of the whole table per row), which otherwise serves tiles whose 46 regions hold
 * more than 512 rows: same bits. */
int chicdiff_hip_region_assemble_dev(chicdiff_hip_ctx *ctx, const int32_t *d_ru_bait, const int32_t *d_ru_oe, int64_t nru,
                                     const int64_t *d_region_ptr, int64_t n, int32_t S, const int64_t *const *d_keys,
                                     const int32_t *const *d_vals, const int64_t *nkeys, int32_t id_min, int32_t nid,
                                     const int64_t *d_midsum, const double *d_sj, const double *d_si, const int32_t *d_tblb,
                                     const int32_t *d_tlb, const double *d_T, int32_t ntblb, int32_t ntlb,
                                     const double *distfun_host, int32_t *d_N, double *d_FullMean);

/* a1, branch without chinput files (chicdiff.R:774-807, = :1202-1260 in getFullRegionData2): N comes from the
 * replicates' Chicago objects.  tempForCounts[[i]] = x[, c("baitID", "otherEndID", "N")] per replicate;
 * mergedFiles <- Reduce(merge, tempForCounts) is merge()'s default INNER join on (baitID, otherEndID), so a pair keeps its
 * counts only when every replicate's table holds it; then merge(RU, ., all.x = TRUE) and N[is.na(N)] <- 0 per replicate.
 * d_keys / d_vals / nkeys are HOST arrays of S entries: one sorted key table per replicate as chicdiff_hip_count_table_dev
 * builds it (device pointers inside).  d_out is nru x S (column s = replicate s). */
int chicdiff_hip_count_join_inner_dev(chicdiff_hip_ctx *ctx, const int32_t *d_ru_bait, const int32_t *d_ru_oe, int64_t nru,
                                      int32_t S, const int64_t *const *d_keys, const int32_t *const *d_vals,
                                      const int64_t *nkeys, int32_t *d_out);

/* a1, branch without chinput files, the merge alone (chicdiff.R:778, the Reduce(merge) of :774-807 and of :1202-1260 in
 * getFullRegionData2):
 *   mergedFiles <- Reduce(merge, tempForCounts)
 * is merge()'s default INNER join on (baitID, otherEndID) over the S replicates' tables: the pairs that EVERY table holds, each
 * with its S counts (N.x, N.y, ... one column per replicate).  It does not depend on the region universe, so one call serves
 * every region set.  A pair is held by a table when its key is there, whatever its count: N = 0 is a count.
 * In: d_keys / d_vals / nkeys, HOST arrays of S entries as in chicdiff_hip_count_join_multi_dev (device pointers inside): one
 * key table per replicate as chicdiff_hip_count_table_dev builds it.  Precondition, as for chicdiff_hip_count_join_dev and
 * not checked: every table's keys are ascending and unique.
 * Out: d_keys_out[0 .. *n_out) = the keys present in all S tables, ascending; d_vals_out[s * cap + i] = table s's value at
 * d_keys_out[i]; *n_out (host) = their number, <= min_s nkeys[s].  Entries from *n_out on are not written.
 * Contract: chicdiff_hip_count_join_multi_dev / chicdiff_hip_region_assemble_dev on the merged tables (d_keys_out with column
 * s, *n_out keys, for replicate s) equal chicdiff_hip_count_join_inner_dev (-> chicdiff_hip_fragment_background_dev ->
 * chicdiff_hip_window_sums_dev) on the original ones bit for bit.
 * The result does not depend on the order of launches or of arrival: rows are placed by a scan, nothing passes through an atomic.
 * Limits: 1 <= S <= 64; cap >= min_s nkeys[s], otherwise CHICDIFF_E_INVALID and nothing is written; no pointer may be NULL
 * (a table's pointers may be where its nkeys is 0, the outputs where the smallest table is empty: then *n_out = 0).  The outputs
 * must not overlap the inputs or each other.  Scratch comes from the context's grow-only workspace.  With timing on the stages
 * are "count_merge_mark", "count_merge_scan" and "count_merge_write". */
int chicdiff_hip_count_tables_merge_dev(chicdiff_hip_ctx *ctx, int32_t S, const int64_t *const *d_keys, const int32_t *const *d_vals,
                                        const int64_t *nkeys, int64_t cap, int64_t *d_keys_out, int32_t *d_vals_out, int64_t *n_out);

/* IHWcorrection's covariate (chicdiff.R:1965-1967 for the test set, :1980-1982 for the control set):
 *   RU.distances <- RU.recast[, list(avDist = mean(distSign)), by = "regionID"]
 * over the long table.  Every (region, fragment) row is repeated once per sample there with the same distSign, so this is
 * the mean over the region's RU rows of CountOut's distSign (chicdiff.R:868-882):
 *   midpoint <- round(0.5 * (start + end))  (per fragment; R's round(), half to even)
 *   distSign <- midpoint[otherEndID] - midpoint[baitID], NA when the fragments lie on different chromosomes.
 * RU rows [d_region_ptr[i], d_region_ptr[i+1]) belong to region i (the CSR chicdiff_hip_region_universe_count_dev
 * returns, or (regionID, otherEndID)-ordered RU rows of any origin).  d_midsum[nid] = start + end of fragment id_min + k;
 * d_chr[nid] = chromosome code (-1 = ID not on the map: such rows are dropped, as merge(x, rmap) drops them) or NULL =
 * all rows cis and on the map.  d_avDist[n]; NaN = NA (a trans row, or no row left).  Pinned by the reference's own
 * result table: its avDist column is reproduced exactly on all 24 863 regions (tests/test_results_postprocessing.py). */
int chicdiff_hip_region_avdist_dev(chicdiff_hip_ctx *ctx, const int32_t *d_ru_bait, const int32_t *d_ru_oe, int64_t nru,
                                   const int64_t *d_region_ptr, int64_t n, int32_t id_min, int32_t nid,
                                   const int64_t *d_midsum, const int32_t *d_chr, double *d_avDist);

/* a3 — per-fragment background, the offset ingredients (chicdiff.R:628-703, 894-896 and Chicago's
 * .estimateBMean/.distFun): for every RU row r = (bait, oe) and replicate s
 *   distSign = round(((start+end)[oe] - (start+end)[bait]) / 2)                         (:648)
 *   Bmean    = s_j[bait] * s_i[oe] * f_s(|distSign|);  s_i NA -> 1;  NA when s_j is NA  (:659-672, 701-702)
 *   Tmean    = T_s[tblb[bait]][tlb[oe]];  tlb NA and tblb known -> min over tlb;  else NA (:676-692)
 *   FullMean = Bmean + Tmean                                                             (:896)
 * Lookup tables are dense over fragment ids [id_min, id_min + nid): d_midsum[nid] (= start+end),
 * and per replicate d_sj, d_si [S][nid] (NaN = absent), d_tblb, d_tlb [S][nid] (-1 = NA),
 * d_T [S][ntblb][ntlb] (NaN = combination absent).  distfun_host[S][10] = cubicFit[0..3],
 * head.coef[0..1], tail.coef[0..1], obs.min, obs.max (chicdiff.R:553-569).  Outputs [S][nru], any
 * may be NULL.  Reading the Chicago objects and the lm() refit stay host R. */
int chicdiff_hip_fragment_background_dev(chicdiff_hip_ctx *ctx, const int32_t *d_bait, const int32_t *d_oe, int64_t nru,
                                         int32_t id_min, int32_t nid, const int64_t *d_midsum, int32_t S,
                                         const double *d_sj, const double *d_si, const int32_t *d_tblb,
                                         const int32_t *d_tlb, const double *d_T, int32_t ntblb, int32_t ntlb,
                                         const double *distfun_host, double *d_bmean, double *d_tmean,
                                         double *d_fullmean);

/* f2 (device part) — chinput columns -> the key table chicdiff_hip_count_join_dev searches:
 * setkey(x, baitID); x <- x[J(baits)] (chicdiff.R:828-831: only rows whose bait is an RU bait) and
 * setkey(temp, baitID, otherEndID) (:849).  d_bait_in_RU: one byte per ID 0..max_id (non-zero = keep) or NULL =
 * keep every row.  d_keys / d_vals hold nrows entries; the first *nkeys_host are the table, ascending in
 * (baitID << 32 | otherEndID), the otherEndID as its 32-bit pattern (a negative one sorts behind the positive ones of its bait; a
 * row with a negative baitID is dropped).  The sort is stable: rows that repeat a (baitID, otherEndID) pair stay in file order, each
 * with its own N.  The joins are written for a table of unique pairs and promise nothing about which of the repeats they return.
 * The chinput text is read by host threads (chicdiff_hip_chinput_read) or, opt-in, parsed on the
 * device (chicdiff_hip_chinput_read_dev); only the header line is host code in both. */
int chicdiff_hip_count_table_dev(chicdiff_hip_ctx *ctx, const int32_t *d_bait, const int32_t *d_oe, const int32_t *d_N,
                                 int64_t nrows, const uint8_t *d_bait_in_RU, int32_t max_id, int64_t *d_keys,
                                 int32_t *d_vals, int64_t *nkeys_host);

/* f2 (text part) — `x <- fread(chinput)` and the column pick `x[, c("baitID", "otherEndID", "N")]` (chicdiff.R:828, :849).
 * _read parses the file with host threads (optional '#' comment lines, a header naming the columns, tab / blank / comma
 * separated integer rows; nthreads <= 0 = the context's default) and keeps the three columns in the context;
 * *nrows_host = rows read.  _table_dev moves them to the device and builds the key table exactly as
 * chicdiff_hip_count_table_dev does (d_keys / d_vals must hold *nrows_host entries). */
int chicdiff_hip_chinput_read(chicdiff_hip_ctx *ctx, const char *path, int32_t nthreads, int64_t *nrows_host);
int chicdiff_hip_chinput_table_dev(chicdiff_hip_ctx *ctx, const uint8_t *d_bait_in_RU, int32_t max_id, int64_t *d_keys,
                                   int32_t *d_vals, int64_t *nkeys_host);

/* limits of the device path of f2's text part (below) */
#define CHICDIFF_CHINPUT_TILE_BYTES 16384    /* consecutive body bytes a workgroup takes in the mark pass and in the parse pass */
#define CHICDIFF_CHINPUT_LANE_BYTES 64       /* consecutive bytes of the tile one lane marks (four 16-byte loads) */
#define CHICDIFF_CHINPUT_WINDOW_BYTES 16640  /* bytes staged in LDS per tile: the tile and an overhang; a line that runs on is read from global memory */
/* f2 (text part) on the device, opt-in: the same rows as chicdiff_hip_chinput_read, parsed by two kernels from the text in device
 * memory.  The rule is the host parser's, stated in full:
 *
 *   header     the leading '#' comment lines and the header line are read on the HOST, exactly as chicdiff_hip_chinput_read reads
 *              them (one function serves both paths): the header's fields are split at tab / blank / comma, a name may be quoted, the
 *              columns may come in any order; ib, io, in = the 0-based positions of baitID, otherEndID, N.  A header that does not
 *              name all three is CHICDIFF_E_INVALID with the host path's message.
 *   body       the bytes after the header line's '\n' (none when the header line is the file's last).
 *   lines      a line runs from a line start — the body's first byte, or the byte after a '\n' — to the next '\n', or to the end of
 *              the body.  ONE trailing '\r' is dropped.  A line that is empty after that is skipped: not a row, not an error.
 *   fields     split at every single tab, blank or comma; two separators in a row make an empty field.
 *   values     only fields ib, io, in are parsed: an optional single '+' or '-', then at least one digit, then digits only; the
 *              magnitude is at most 2147483647 (so -2147483648 is malformed).  Scanning stops after the largest of the three
 *              positions: whatever follows on the line is never looked at, however long.  A line on which fewer than three of them were
 *              found is malformed.
 *   output     rows in file order.  Any malformed line fails the call; the offset reported is that of the SMALLEST malformed line
 *              start.
 * Row r's place is the number of non-blank line starts before it, from one scan of per-tile counts and one inside the tile: no value
 * passes through an atomic, and launch shape and arrival order cannot show in the result (the one atomic is a 64-bit minimum over
 * the offsets of malformed lines).
 *
 * _parse_dev: the device stage alone.  d_text: the body, nbytes >= 0 bytes of device memory, 16-byte aligned; ib, io, in >= 0 and
 * distinct; d_bait, d_oe, d_N: room for `cap` rows.  *nrows_host = the rows of the body.  nrows > cap: CHICDIFF_E_INVALID before
 * anything is written (the count is known before the parse pass starts).  A malformed line: CHICDIFF_E_INVALID, *bad_offset_host =
 * its body-relative offset (-1 otherwise), message `malformed chinput row at byte offset K (...)`; the rows' contents are then
 * unspecified.  One host stop for the count, one for the verdict.
 * _read_dev: header on the host, the body through a bounded pinned staging area to the device (host_copy_threads threads copy
 * chunks into its two halves; the DMA of one half runs while the other is filled), then the stage above.  The text and the three
 * columns stay in grow-only buffers of the context (released by chicdiff_hip_destroy), apart from every workspace:
 * chicdiff_hip_chinput_table_dev then builds the key table from them with no host copy.  The context remembers which of _read and
 * _read_dev came last, and _table_dev serves that one.  Messages are the host path's (`cannot open ...`, `empty file`, the header
 * message, `malformed chinput row at byte offset K (...)` with K counted from the start of the FILE); an allocation that fails is
 * CHICDIFF_E_NOMEM, the message naming the file size.
 * chicdiff_hip_chinput_caps: the three constants above, as the library was built (any pointer may be NULL); host only, no context. */
int chicdiff_hip_chinput_parse_dev(chicdiff_hip_ctx *ctx, const uint8_t *d_text, int64_t nbytes, int32_t ib, int32_t io, int32_t in,
                                   int32_t *d_bait, int32_t *d_oe, int32_t *d_N, int64_t cap, int64_t *nrows_host,
                                   int64_t *bad_offset_host);
int chicdiff_hip_chinput_read_dev(chicdiff_hip_ctx *ctx, const char *path, int64_t *nrows_host);
int chicdiff_hip_chinput_caps(int32_t *tile_bytes, int32_t *lane_bytes, int32_t *window_bytes);

/* limits and words of the device path of readAndFilterPeakMatrix (below) */
#define CHICDIFF_PEAKS_KEY_COLUMNS 11    /* baitChr baitStart baitEnd baitID baitName oeChr oeStart oeEnd oeID oeName dist, by position */
#define CHICDIFF_PEAKS_MAX_SCORES 64     /* score columns one read takes */
#define CHICDIFF_PEAKS_MAX_SLOW 65536    /* decimal tokens per read that the device may leave to the host's strtod */
#define CHICDIFF_PEAKS_ST_QUOTE 1        /* status bit: the body holds a '"' — nothing was parsed */
#define CHICDIFF_PEAKS_ST_SLOW_OVERFLOW 2 /* status bit: more slow tokens than the list holds — the columns are not complete */
/* info[CHICDIFF_PEAKS_INFO_WORDS] of the calls below (int64 each) */
#define CHICDIFF_PEAKS_INFO_NROWS 0      /* rows of the body */
#define CHICDIFF_PEAKS_INFO_STATUS 1     /* CHICDIFF_PEAKS_ST_* bits; non-zero: the caller reads the file some other way */
#define CHICDIFF_PEAKS_INFO_MAXBAIT 2    /* largest baitID, -1 without rows */
#define CHICDIFF_PEAKS_INFO_NSLOW 3      /* decimal tokens settled by the host */
#define CHICDIFF_PEAKS_INFO_BAD 4        /* body offset of the first malformed line, -1 = none */
#define CHICDIFF_PEAKS_INFO_BODY 5       /* file offset of the body (_read_dev, _selftest_peaks; 0 for _parse_dev) */
#define CHICDIFF_PEAKS_INFO_SEP 6        /* the separator byte */
#define CHICDIFF_PEAKS_INFO_NSCORE 7     /* score columns */
#define CHICDIFF_PEAKS_INFO_NKEPT 8      /* _selftest_peaks: rows the filter keeps */
#define CHICDIFF_PEAKS_INFO_NFILTERED 9  /* _selftest_peaks: baits without a kept row */
#define CHICDIFF_PEAKS_INFO_WORDS 10
/* readAndFilterPeakMatrix (chicdiff.R:218-277) on the device, opt-in: x <- fread(peakFiles); x[, c(1:11, sel)] (:231-244); the four
 * filters (:246-270); filtered baits (:240, :271).  One peak file per read; .multimerge (:223-229) is
 * chicdiff_hip_peaks_merge_dev, further down.  The rule, in full:
 *
 *   header     read on the HOST.  Leading '#' lines are skipped; the next line is the header, one trailing '\r' dropped.  The separator
 *              is ONE byte for the whole file: a tab if the header line holds a tab, else a comma if it holds a comma, else a blank.
 *              Header fields are split at every separator byte; a name may be quoted.  Fields 0 .. 10 must be exactly baitChr,
 *              baitStart, baitEnd, baitID, baitName, oeChr, oeStart, oeEnd, oeID, oeName, dist in that order (the reference takes them
 *              by position and uses them by name).  The score columns are the fields from 11 on whose names are targetColumns, in
 *              FILE order.  Refused with a message (CHICDIFF_E_INVALID): a target that no field from 11 on names ("All specified
 *              targetColumns must be present in the peak file(s)", the reference's words, :232); a target named twice (in the list or
 *              in the header); a target that is one of the 11 key names; more than CHICDIFF_PEAKS_MAX_SCORES targets.
 *   body       the bytes after the header line's '\n'.
 *   lines      as for chinput, unchanged: a line starts at the body's first byte or after a '\n' and runs to the next '\n' or the
 *              body's end; ONE trailing '\r' is dropped; a line that is empty after that is skipped.
 *   fields     split at every single separator byte; two in a row make an empty field, and a separator as the line's last byte is
 *              followed by an empty field.  A body that holds a '"' ANYWHERE is not parsed: CHICDIFF_PEAKS_ST_QUOTE, no row written.
 *   integers   fields 1, 2, 3, 6, 7, 8 (baitStart, baitEnd, baitID, oeStart, oeEnd, oeID): chinput's rule — an optional single '+' or
 *              '-', at least one digit, digits only, magnitude <= 2147483647.  NA is malformed.  baitID and oeID are >= 0.
 *   decimals   field 10 (dist) and every score column.  Empty, or exactly NA: NaN.  Otherwise the token is
 *                  [+-]? (d+ (. d*)? | . d+) ([eE] [+-]? d+)?
 *              and the value is the double nearest to the decimal number it writes, ties to even — what strtod and Python's float()
 *              return, bit for bit, signed zero included.  Anything else is malformed.
 *   text       fields 0, 4, 5, 9 and every field that is no score column are skipped byte-wise, never interpreted.
 *   malformed  nothing behind the last needed field (the last score column; dist without score columns) is looked at.  A line with
 *              fewer fields than that is malformed.  Any malformed line fails the call with `malformed peak matrix row at byte offset
 *              K (...)`, K the SMALLEST malformed line start (a 64-bit atomicMin).
 *   filter     a row is kept when (1) some score column is > score (NaN never is); (2) if replicate_rule != 0 (more target columns than
 *              conditions, :253), every condition c in 0 .. ncond-1 has >= 2 non-NaN values among the score columns j with
 *              cond_of_col[j] == c; (3) dist is not NaN; (4) oeID != baitID + 1 and oeID != baitID - 1, compared in 64 bits.
 *   output     the kept rows' indices in FILE order with their baitID / oeID gathered, and the filtered baits: the baitIDs that occur
 *              in the file and have no kept row, in order of FIRST APPEARANCE in the file (all_baits <- unique(x$baitID), then %in%).
 *
 * Decimal -> double on the device (peaks_decimal.h): the token is (w, q), w its digits up to the last non-zero one without leading
 * zeros, value = w * 10^q.  For w of at most 19 digits and |q| <= 39 the rounding is decided exactly from integers of at most 192
 * bits.  Any other non-zero token is a SLOW token: its cell and offset go on a list of CHICDIFF_PEAKS_MAX_SLOW entries (one counter;
 * every cell is patched on its own, so the slot order cannot show), the host settles it with strtod and a kernel writes the cells
 * before the call returns; more than the list holds: CHICDIFF_PEAKS_ST_SLOW_OVERFLOW.  A token with at most 17 significant digits
 * and |q| <= 22 — what shortest-round-trip writers produce for Chicago scores — is never slow.
 * Row r's place comes from the two scans alone, as for chinput; the kept rows' and filtered baits' places from one scan of packed
 * flags.  No value passes through an atomic.
 *
 * _parse_dev: the device stage alone, for tests.  d_text: the body, 16-byte aligned; sep the separator byte; score_cols[nscore] (host):
 * the score columns' 0-based fields, ascending, >= 11.  d_ints (6, cap) int32: baitStart, baitEnd, baitID, oeStart, oeEnd, oeID;
 * d_dist (cap); d_scores (nscore, cap); d_line_off (cap): the body offset of every row's line.  info (host): the words above.  More
 * rows than cap: CHICDIFF_E_INVALID before anything is written, info[NROWS] set.  A status bit: CHICDIFF_OK, nothing usable written.
 * Host stops: the row count (with the quote verdict); the verdict (malformed offset, max baitID, slow count).
 * _read_dev: header on the host (targets[ntargets]: the targetColumns), the body through the bounded pinned area of
 * chicdiff_hip_chinput_read_dev to the device, then the stage above into grow-only buffers of the context, apart from every
 * workspace.  score_target[j] (host, room for ntargets): which target score row j is.  Offsets in messages count from the start of
 * the FILE.  _columns_dev copies the context's columns of the last successful _read_dev into the caller's (shapes as for _parse_dev).
 * _filter_dev: d_bait, d_oe, d_dist (n), d_scores (nscore, n); cond_of_col[nscore] (host), maxbait = info[MAXBAIT] (any bound on
 * baitID will do; the bait table has maxbait + 1 words of 8 bytes in the context's grow-only workspace and is cleared by a memset, so ONE
 * stray large ID costs device memory in proportion: 16 GiB at the largest legal ID, 2^31 - 1; CHICDIFF_E_NOMEM when that fails).  d_kept_idx (int64), d_kept_bait, d_kept_oe, d_filtered (int32): room for n
 * each; *nkept_host / *nfiltered_host entries are written.  One host stop.
 * _caps: the tile and window (the chinput constants) and the two limits above, as the library was built; host only. */
int chicdiff_hip_peaks_parse_dev(chicdiff_hip_ctx *ctx, const uint8_t *d_text, int64_t nbytes, int32_t sep, const int32_t *score_cols,
                                 int32_t nscore, int32_t *d_ints, double *d_dist, double *d_scores, int64_t *d_line_off, int64_t cap,
                                 int64_t *info);
int chicdiff_hip_peaks_read_dev(chicdiff_hip_ctx *ctx, const char *path, const char *const *targets, int32_t ntargets,
                                int32_t *score_target, int64_t *info);
int chicdiff_hip_peaks_columns_dev(chicdiff_hip_ctx *ctx, int32_t *d_ints, double *d_dist, double *d_scores, int64_t *d_line_off,
                                   int64_t cap);
int chicdiff_hip_peaks_filter_dev(chicdiff_hip_ctx *ctx, const int32_t *d_bait, const int32_t *d_oe, const double *d_dist,
                                  const double *d_scores, int64_t n, int32_t nscore, double score, const int32_t *cond_of_col,
                                  int32_t ncond, int32_t replicate_rule, int64_t maxbait, int64_t *d_kept_idx, int32_t *d_kept_bait,
                                  int32_t *d_kept_oe, int32_t *d_filtered, int64_t *nkept_host, int64_t *nfiltered_host);
int chicdiff_hip_peaks_caps(int32_t *tile_bytes, int32_t *window_bytes, int32_t *max_scores, int32_t *max_slow);

/* .multimerge on the device, opt-in (chicdiff.R:218-228, 234-236): peakfiles names F >= 2 files and the reference joins them with
 * Reduce(merge(..., all = TRUE)) on the eleven key columns.  The twin is pandas' x.merge(y, on = the 11 keys, how = "outer"), left to
 * right.  Words and limits: */
#define CHICDIFF_PEAKS_MERGE_MAX_FILES 16
#define CHICDIFF_PEAKS_ST_CHR_LONG 4          /* status bit: a text chromosome token over 8 bytes (or a 9-digit number in a text column) */
#define CHICDIFF_PEAKS_ST_CHR_AMBIGUOUS 8     /* status bit: a chromosome token that is neither a plain integer nor text */
#define CHICDIFF_PEAKS_ST_MERGE_DUPLICATE 16  /* status bit: two rows of one file share their eight words */
#define CHICDIFF_PEAKS_ST_MERGE_NAME 32       /* status bit: rows that share a bait (a key) differ in baitName (oeName) */
#define CHICDIFF_PEAKS_ST_MERGE_DIST 64       /* status bit: rows that share their eight words differ in dist */
#define CHICDIFF_PEAKS_KEY_INT 0              /* a chromosome column's class: every row a plain integer (pandas: int64) */
#define CHICDIFF_PEAKS_KEY_TEXT 1             /* every row text (pandas: object) */
#define CHICDIFF_PEAKS_KEY_MIXED 2            /* plain integers and text: object for pandas too, ordered as strings like TEXT */
#define CHICDIFF_PEAKS_TEXTKEYS_STATUS 0      /* info[] of _textkeys_dev / _selftest_peaks_textkeys: CHICDIFF_PEAKS_ST_CHR_* bits */
#define CHICDIFF_PEAKS_TEXTKEYS_CLASS_BAIT 1  /* class of baitChr */
#define CHICDIFF_PEAKS_TEXTKEYS_CLASS_OE 2    /* class of oeChr */
#define CHICDIFF_PEAKS_TEXTKEYS_NROWS 3
#define CHICDIFF_PEAKS_TEXTKEYS_WORDS 4
#define CHICDIFF_PEAKS_MERGE_NOUT 0           /* info[] of _merge_dev: rows of the merged table */
#define CHICDIFF_PEAKS_MERGE_STATUS 1         /* CHICDIFF_PEAKS_ST_MERGE_* bits; non-zero: the merged table must not be used */
#define CHICDIFF_PEAKS_MERGE_WORDS 2
/* The rule, in full.
 *
 *   twin's order   pandas returns the outer join ordered lexicographically by the eleven key columns; regionID is the row number of
 *                  the filtered table (:393), so the order is part of the result.  A baitChr / oeChr column that pandas types object
 *                  orders as strings ("10" < "2" < "X"), one it types int64 numerically; int64 in one file against object in another
 *                  raises.  NA dist keys (trans rows) match each other.  Two rows of one file with one key give a Cartesian product.
 *   eight words    (chr(baitChr), baitStart, baitEnd, baitID, chr(oeChr), oeStart, oeEnd, oeID).  If no two rows that agree in them
 *                  differ in baitName, oeName or dist, and no two rows that agree in the first four differ in baitName, the twin's
 *                  order is the order of these words.  The device sorts on exactly them, checks the condition, and reports a status
 *                  bit where it fails: the caller then reads the files some other way.
 *   chr()          a chromosome token is one of
 *                    plain integer  0|[1-9][0-9]{0,8}; the key is its value.
 *                    text           1 .. 8 bytes, every byte ASCII, at least one byte outside 0-9 + - . e E and blank, not one of
 *                                   pandas' NA spellings ('' #N/A '#N/A N/A' #NA -1.#IND -1.#QNAN -NaN -nan 1.#IND 1.#QNAN <NA> N/A NA
 *                                   NULL NaN None n/a nan null), not [+-]?(inf|infinity) in any letter case; the key is the bytes
 *                                   packed big-endian, zero-padded, the top bit flipped: signed int64 order is byte order.
 *                    anything else  CHICDIFF_PEAKS_ST_CHR_LONG for a token over 8 bytes that is text otherwise,
 *                                   CHICDIFF_PEAKS_ST_CHR_AMBIGUOUS for the rest (01, +1, 1.0, 1e5, inf, an NA spelling, a non-ASCII
 *                                   byte, ten or more digits).
 *                  A column's class follows its rows: all plain integers INT; else TEXT or MIXED, and then EVERY row's key is its
 *                  bytes (['1', '2L'] is object for pandas), which a 9-digit number does not fit: CHR_LONG.
 *   names          baitName and oeName enter as 64-bit FNV-1a hashes of the field's bytes.  Equal bytes give equal hashes; unequal
 *                  bytes give equal hashes with probability 2^-64 per pair, and such a pair would pass as one name.
 *   groups         rows are concatenated file-major and a permutation is sorted by the eight words with stable radix passes, so a
 *                  group's members stand in file order.  A sorted row opens a group when any word differs from its predecessor's.
 *                  Inside a group: two rows of one file DUPLICATE, unequal oeName hashes NAME, unequal dist DIST (NaN equals NaN,
 *                  +0 equals -0).  Along a run of equal (chr(baitChr), baitStart, baitEnd, baitID): unequal baitName hashes NAME.
 *   output         one row per group, in sorted order: the six ints and dist of the group's first member, src_file / src_row of that
 *                  member (the text columns are cut from that file), and the (sum T_f, n_out) score matrix: file f's score rows at
 *                  sum_{g < f} T_g, NaN where file f has no such key — the twin's column order.
 *
 * _textkeys_dev works on the body of the last successful _read_dev of this context, still in the context's text buffer (any other
 * read through the context in between: CHICDIFF_E_INVALID).  One lane per row walks fields 0 .. 9 from the row's line offset.
 * d_chr (2, cap) int64: chr(baitChr), chr(oeChr) in the form of each column's class; d_name (2, cap): the hashes of baitName, oeName;
 * cap >= the rows of that read.  info (host): the words above.  One host stop (the flag words).
 * _merge_dev: nfiles in 2 .. CHICDIFF_PEAKS_MERGE_MAX_FILES; per file (host arrays of device pointers) d_ints (6, n_f) int32, d_dist
 * (n_f), d_scores (T_f, n_f), d_chr and d_name (2, n_f) as above, all contiguous; nrows[f] = n_f >= 0, nscores[f] = T_f >= 0, sum T_f <=
 * CHICDIFF_PEAKS_MAX_SCORES, sum n_f < 2^31.  The caller has made sure that every file's columns have one class (INT everywhere, or
 * TEXT / MIXED everywhere).  Outputs (device, cap >= sum n_f columns each): d_out_ints (6, cap), d_out_dist (cap), d_out_scores (sum
 * T_f, cap), d_src_file (cap) int32, d_src_row (cap) int64; the first info[NOUT] columns are written.  One host stop.  The result
 * does not depend on the launch shape: no value passes through an atomic, only status bits do.
 * _header (host only, no context): the header of a file through the same function as _read_dev's, without targets: the column names
 * joined by '\n' into names (namecap bytes, NUL-terminated), *ncols their number, *sep the separator byte.  A file whose first 11
 * columns are not the key columns is refused with that function's message in err. */
int chicdiff_hip_peaks_textkeys_dev(chicdiff_hip_ctx *ctx, int64_t *d_chr, int64_t *d_name, int64_t cap, int64_t *info);
int chicdiff_hip_peaks_merge_dev(chicdiff_hip_ctx *ctx, int32_t nfiles, const int32_t *const *d_ints, const double *const *d_dist,
                                 const double *const *d_scores, const int64_t *const *d_chr, const int64_t *const *d_name,
                                 const int64_t *nrows, const int32_t *nscores, int64_t cap, int32_t *d_out_ints, double *d_out_dist,
                                 double *d_out_scores, int32_t *d_src_file, int64_t *d_src_row, int64_t *info);
int chicdiff_hip_peaks_header(const char *path, char *names, int32_t namecap, int32_t *ncols, int32_t *sep, char *err, int32_t errcap);
/* _selftest_peaks_textkeys (host only, no context): the host statement of the text-key rule on a file — header as above, the body
 * parsed by the host statement of the parse rule (no targets), then chr (2, cap) and name (2, cap) as _textkeys_dev gives them, for the
 * first min(nrows, cap) rows; info as for _textkeys_dev.  cap = 0: the row count alone. */
int chicdiff_hip_selftest_peaks_textkeys(const char *path, int64_t cap, int64_t *chr, int64_t *name, int64_t *info, char *err, int32_t errcap);

/* f1/f3 — p.adjust(p, method = "BH") (DESeq2 results() on the independent-filtering survivors; chicdiff.R:2049
 * on the weighted p-values).  NaN = NA: not counted, stays NaN.  n < 2^32. */
int chicdiff_hip_bh_adjust_dev(chicdiff_hip_ctx *ctx, const double *d_p, int64_t n, double *d_padj);

/* a9 — DESeq2 results() on device (chicdiff.R:1720-1741 call it with its defaults).
 *
 * Cook's cutoff: p <- NA where maxCooks > cutoff (host passes qf(.99, p, m - p)); for the two-group design the
 * p-value is kept when at least 3 counts of the row exceed the count of the sample with the largest Cook's
 * distance.  Only meaningful when some group has >= 3 samples (otherwise DESeq2 skips the step: do not call).
 * d_pvalue is modified in place; *n_outliers_host = rows set to NA. */
int chicdiff_hip_cooks_filter_dev(chicdiff_hip_ctx *ctx, const int32_t *d_counts, int64_t n, int32_t S, const int32_t *group,
                                  const double *d_maxCooks, const int32_t *d_cooksArgmax, double cutoff, double *d_pvalue,
                                  int64_t *n_outliers_host);

/* Independent filtering + BH (pvalueAdjustment, independentFiltering = TRUE): theta = seq(mean(baseMean == 0), 0.95,
 * length = 50), cutoffs = quantile(baseMean, theta), numRej[k] = #{BH-adjusted p < alpha among rows with baseMean >=
 * cutoff k}, lowess(numRej ~ theta, f = 1/5), first theta whose numRej exceeds max(fit) - RMSE; padj = BH over the rows
 * passing that cutoff, NaN elsewhere. */
typedef struct {
    double filterThreshold, filterTheta, alpha;
    int32_t index; /* 1-based position of the chosen theta */
    int32_t _pad;
    double theta[50], numRej[50], lowess[50];
} chicdiff_results_info;
/* A NaN baseMean is refused (CHICDIFF_E_INVALID): R's quantile() stops on missing values. */
int chicdiff_hip_independent_filtering_dev(chicdiff_hip_ctx *ctx, const double *d_baseMean, const double *d_pvalue, int64_t n,
                                           double alpha, double *d_padj, chicdiff_results_info *info);

/* f3 — application side of IHWcorrection (chicdiff.R:2038-2049), after ihw() has been trained in R:
 *   group <- as.integer(cut(log(abs(avDist)), breaks)); avWeights <- distLookup$avWeights[group];
 *   weight <- avWeights / mean(avWeights); weighted_pvalue <- pvalue / weight;
 *   weighted_padj <- p.adjust(weighted_pvalue, "BH").
 * breaks_host has ngroups + 1 ascending entries (chicdiff.R:2039), avWeights_host ngroups (<= 256).
 * d_group gets 1-based codes, INT32_MIN (NA_integer_) outside the breaks; any output may be NULL except
 * d_weighted_padj. */
int chicdiff_hip_ihw_apply_dev(chicdiff_hip_ctx *ctx, const double *d_avDist, const double *d_pvalue, int64_t n,
                               const double *breaks_host, const double *avWeights_host, int32_t ngroups,
                               int32_t *d_group, double *d_weight, double *d_weighted_pvalue,
                               double *d_weighted_padj);

/* limits of chicdiff_hip_ihw_train_dev (below) */
#define CHICDIFF_IHW_MAX_BINS 256      /* ihw_apply's own limit */
#define CHICDIFF_IHW_MAX_FOLDS 16
#define CHICDIFF_IHW_PHILOX_STREAM 16u /* counter word 3 of the fold draws (the control draws use streams 0 and 1) */
typedef struct {
    int64_t m;         /* kept rows */
    int32_t nbins;     /* the number of groups used */
    int32_t nfolds;
    int32_t chunk_len; /* IN: 0 = the default, or one of chicdiff_hip_ihw_caps' chunk lengths (results never depend on it); OUT: the one used */
    int32_t _pad;
    int64_t nseg[CHICDIFF_IHW_MAX_FOLDS]; /* segments of all groups, per fold */
    double T[CHICDIFF_IHW_MAX_FOLDS];     /* step 5's T and H, per fold */
    double H[CHICDIFF_IHW_MAX_FOLDS];
} chicdiff_ihw_info;
/* Training side of IHWcorrection: ihw(pvalue ~ abs(avDist), data = out.control, alpha = 0.05) (chicdiff.R:1994), as far as distLookup
 * (:2012-2031) reads its result: the group of every row and the nbins x nfolds weight matrix.  This is THIS LIBRARY'S STATEMENT of
 * independent hypothesis weighting, not a port of the IHW package (differences below).  Every operation of the rule is an integer
 * operation, an IEEE double + - * / in the stated order (the library is built with -ffp-contract=off) or an exact comparison: the
 * result is a pure function of the inputs, the same bits on every run, chunk length and launch shape.
 *
 * Inputs: d_pvalue[n], d_covariate[n] (device, float64), alpha in (0, 1), nbins (0 = auto), nfolds, a 64-bit seed.
 *
 * 1. Kept rows.  A row whose p-value is NaN is left out: its group is INT32_MIN and its fold -1, whatever its covariate.  m = the
 *    number of kept rows.  A p-value of -0 is taken as +0.  nbins = 0 means max(1, min(40, m / 1500)) in integer division.  Limits:
 *    1 <= nbins <= min(m, CHICDIFF_IHW_MAX_BINS), 2 <= nfolds <= CHICDIFF_IHW_MAX_FOLDS, n * nfolds < 2^31.
 * 2. Groups (groups_by_filter: ceiling(rank(cov, ties = "first") / m * nbins)).  r_i = 1 + the number of kept rows that precede row i
 *    in the stable order by covariate: -0 and +0 are equal, +Inf sorts last, ties go by row index.
 *    group_i = ceil(((double)r_i / (double)m) * (double)nbins): exactly these two double operations; groups are 1-based.
 * 3. Folds.  fold_i = ((uint64)w0 * nfolds) >> 32, w0 = word 0 of philox4x32_10(counter = (i & 0xffffffff, i >> 32, 0,
 *    CHICDIFF_IHW_PHILOX_STREAM), key = (seed & 0xffffffff, seed >> 32)) (the generator of chicdiff_hip_control_draws_dev); i is the
 *    row's index in the caller's array, so a row's fold does not depend on which rows are NA.
 * 4. Grenander estimator of (fold f, group g).  P = the p-values of the kept rows of group g whose fold is NOT f, M = |P|.  The points
 *    are (0, 0), then (u, c(u)) for every distinct u in P with c(u) = #{p in P: p <= u}, then (1, M); of points with equal x only the
 *    one with the largest count is a point.  The knots are the vertices of the least concave majorant of the points: a point b between
 *    its neighbours a and c (of the knots) is a knot iff (b.c - a.c) * (c.x - a.x) > (c.c - a.c) * (b.x - a.x) IN EXACT ARITHMETIC —
 *    collinear points are not knots.  M = 0: the knots are (0, 0), (1, 1), and M is taken as 1.  Per segment j between consecutive
 *    knots j - 1 and j, in double, in this order: d = x_j - x_{j-1}; dF = (double)(c_j - c_{j-1}) / (double)M; s = dF / d.
 *    F(0) = (double)c_0 / (double)M, c_0 the count of the first knot (positive when P holds zeros).
 * 5. Weights of fold f.  h_g = the kept rows of group g IN fold f, H = sum h_g (integers).  All segments of all groups are put in the
 *    order (s descending, g ascending, j ascending).  B = 0; for g = 1, 2, ..: B = B - (alpha * (double)h_g) * F_g(0).  Walking the
 *    order: cost = (double)h_g * (d - alpha * dF); while B + cost <= 0 the whole segment is taken: t_g = t_g + d, B = B + cost; at the
 *    first segment where that fails t_g = t_g + (-B / cost) * d, and the walk stops.  T = sum_g (double)h_g * t_g, summed in group
 *    order from 0.  w[g][f] = (t_g * (double)H) / T; T = 0 (H = 0 included): every weight of the fold is 1.
 *    This is the exact optimum of IHW's linear programme without a regularisation term (maximise sum h_g F_g(t_g) subject to
 *    sum h_g t_g <= alpha sum h_g F_g(t_g)): a fractional knapsack over segments ordered by slope.
 *
 * Differences from the package: no total-variation penalty and no nested cross-validation over lambdas (the rule is the package's
 * with lambdas = Inf); folds from this library's Philox stream, not R's sample() under set.seed(1); no null-proportion adjustment;
 * no adjusted p-values (Chicdiff discards them).  On null data the unregularised weights are valid through cross-weighting but erratic.
 *
 * Outputs: d_group[n], d_fold[n] (device int32; d_fold may be NULL); weights_host[nbins x nfolds], R's column-major matrix
 * (w[g][f] at [g - 1 + nbins * f]); *info (its chunk_len is read first).  Everything is enqueued on the context's stream, with two host
 * stops: the read of the verdicts and the segment total (which sizes the sort by slope), and the read of the weights and of info.
 * CHICDIFF_E_INVALID, the message naming the cause and, where there is one, the row: a p-value outside [0, 1]; a NaN covariate on a
 * kept row; no kept row; nbins > m or > CHICDIFF_IHW_MAX_BINS; nfolds outside its limits; alpha outside (0, 1); a chunk length not in
 * chicdiff_hip_ihw_caps' list.  On a refusal the outputs are unspecified. */
int chicdiff_hip_ihw_train_dev(chicdiff_hip_ctx *ctx, const double *d_pvalue, const double *d_covariate, int64_t n, double alpha,
                               int32_t nbins, int32_t nfolds, uint64_t seed, int32_t *d_group, int32_t *d_fold, double *weights_host,
                               chicdiff_ihw_info *info);
/* The limits above, the largest automatic nbins, and the chunk lengths the library accepts (up to `cap` of them into chunk_lens,
 * ascending, the last being the default; *nchunk_lens = how many there are).  Every pointer may be NULL. */
int chicdiff_hip_ihw_caps(int32_t *max_bins, int32_t *max_folds, int32_t *auto_max_bins, int32_t *chunk_lens, int32_t cap,
                          int32_t *nchunk_lens);

/* f4 — getRegionUniverse, window mode (chicdiff.R:353-426).  For peak i (regionID i + 1): the otherEndIDs
 * .expandAvoidBait(baitID, oeID, RUexpand) (:353-367), kept when 1 <= ID <= maxfrag (:383-384) and on the bait's
 * chromosome (:386-401).  d_chr_of[0 .. maxfrag]: chromosome code of each restriction-map ID (-1 = ID not on
 * the map; entry 0 unused).  Two calls: _count fills d_region_ptr[n + 1] (CSR offsets), optional d_minOE /
 * d_maxOE (INT32_MIN for an empty region) and *total_host = number of RU rows; _fill writes the rows in
 * (regionID, otherEndID) order — RU.DT's own order is the stable sort of these rows by baitID after
 * otherEndID (setkey, :389/:393).  baitID == oeID is the reference's stop("Invalid parameters"): E_INVALID.
 *
 * IDs off the map, at any int32 value (this holds for _count, _fill and the one call alike): d_bait and d_oe may hold every int32,
 * INT32_MIN and INT32_MAX included.  The window is formed in 64-bit arithmetic and clamped to the map, [1, maxfrag]; IDs outside the
 * map are never kept, so the clamp changes no row.  A peak whose window misses the map, or whose bait is not on it, gives an empty
 * region (no rows, INT32_MIN in d_minOE / d_maxOE) and no refusal; baitID == oeID is refused whatever the ID.  The reference itself
 * stops short of this: R's integer arithmetic gives NA where oeID + RUexpand or baitID + 2 overflows, and `NA:b` is an error.
 * Limit: 1 <= maxfrag < 2^30 (a larger one is E_INVALID, the message naming the limit): with the window inside the map no 32-bit
 * counter over it can overflow. */
int chicdiff_hip_region_universe_count_dev(chicdiff_hip_ctx *ctx, const int32_t *d_bait, const int32_t *d_oe, int64_t n,
                                           int32_t RUexpand, const int32_t *d_chr_of, int32_t maxfrag,
                                           int64_t *d_region_ptr, int32_t *d_minOE, int32_t *d_maxOE,
                                           int64_t *total_host);
int chicdiff_hip_region_universe_fill_dev(chicdiff_hip_ctx *ctx, const int32_t *d_bait, const int32_t *d_oe, int64_t n,
                                          int32_t RUexpand, const int32_t *d_chr_of, int32_t maxfrag,
                                          const int64_t *d_region_ptr, int32_t *d_ru_bait, int32_t *d_ru_region,
                                          int32_t *d_ru_oe);
/* ... both in ONE call: the caller gives room for the upper bound `capacity` >= n max(2 RUexpand + 1, 2) rows in the three row vectors
 * (the first *total_host of them are written; two rows per peak for RUexpand = 0: R's descending (bait + 2):(oe + 0) beside a bait,
 * chicdiff.R:359-363), so that nothing on the host stands between the scan and the fill. */
int chicdiff_hip_region_universe_dev(chicdiff_hip_ctx *ctx, const int32_t *d_baitID, const int32_t *d_oeID, int64_t n, int32_t RUexpand,
                                     const int32_t *d_chr_of, int32_t maxfrag, int64_t *d_region_ptr, int32_t *d_minOE,
                                     int32_t *d_maxOE, int32_t *d_ru_baitID, int32_t *d_ru_regionID, int32_t *d_ru_otherEndID,
                                     int64_t capacity, int64_t *total_host);

/* getCandidateInteractions (chicdiff.R:2068-2163): the region-level results turned into fragment-level candidate interactions —
 * setkey(output, baitID, minOE, maxOE), the overlap join of every peak row against the regions of its bait (foverlaps, :2129),
 * min(pcol) per (baitID, oeID) group and the final filter (:2161).  No work is done on host buffers; everything is enqueued on
 * the context's stream, and the only host stop is the read of the two counts.
 *
 * Inputs (device): the region table in the caller's row order (= rows of `output`, any order) as d_baitID, d_minOE, d_maxOE
 * (int32[n]) and d_p (double[n], the chosen pcol, NaN = NA); the peak matrix's rows as read, BEFORE the score filter, as
 * d_peak_baitID, d_peak_oeID (int32[npeaks]) and d_scores (double[npeaks x ncols], column-major, NaN = NA): the first ncond1
 * columns are condition 1, the next ncond2 condition 2; merged = 1 (a merged peak matrix) asks for ncond1 = ncond2 = 1.
 *
 * Rules, by statement of the reference:
 *   selection (:2082-2087)   a peak row is selected when some score column is > score and not NA.
 *   delta (:2118-2124)       |asinh(mean of the cond-1 columns) - asinh(mean of the cond-2 columns)|.  rowMeans has no na.rm: one NA
 *                            makes delta NA.  Each row sum is formed as a double-double and rounded once, then divided once; R's
 *                            rowMeans accumulates in long double, and agreement with that 80-bit sum in the last bit is unpinned.
 *   delta, merged (:2126)    |col2 - col1| with NO asinh — what the reference computes for a merged peak matrix, kept as it is.
 *   overlap (:2129)          type = "any" on the closed point interval [oe, oe]: peak and region match when baitID is equal and
 *                            minOE <= oeID <= maxOE.  nomatch = 0: a peak without a region forms no group.
 *   min_p (:2145)            min(pcol) over the group's regions WITHOUT na.rm: any NaN gives NaN.
 *   filter (:2161)           min_p <= pvcut & delta >= minDeltaAsinhScore; a NaN on either side drops the group.  The filter runs on
 *                            the device: only surviving groups get a slot, a CSR entry and pairs.
 *
 * Outputs (device): d_group_peak (int32[npeaks]) the peak row of each surviving group, groups in ascending (baitID, oeID) order;
 * d_group_ptr (int64[npeaks + 1]) CSR offsets into the pairs; d_group_min_p, d_group_delta (double[npeaks]); d_pair_row
 * (int32[pair_capacity]) rows of the region table, within a group ordered by (minOE, maxOE), ties in order of appearance in the
 * table (setkey is a stable sort, and foverlaps(mult = "all") returns matches in key order).  *ngroups_host, *npairs_host: how many
 * entries are written.
 *
 * The number of pairs has no a-priori bound (duplicate regions are legal).  When it exceeds pair_capacity the call writes both counts
 * and everything per group, writes NO pair, and returns CHICDIFF_E_INVALID with a message that names the need: call again with
 * that much room.
 *
 * CHICDIFF_E_INVALID, the message naming the offending row: a region row with minOE > maxOE or an INT32_MIN (NA) key (foverlaps stops
 * on both); two SELECTED peak rows with the same (baitID, oeID) (the reference would merge them into one group; Chicago's peak
 * matrix has one row per pair); a selected peak row with baitID = oeID = INT32_MAX.  Also n < 1, n >= 2^31, ncols < 2,
 * npeaks >= 2^31.  npeaks = 0 or no survivor: CHICDIFF_OK with zero groups (d_group_ptr[0] = 0). */
int chicdiff_hip_candidate_interactions_dev(chicdiff_hip_ctx *ctx, const int32_t *d_baitID, const int32_t *d_minOE, const int32_t *d_maxOE,
                                            const double *d_p, int64_t n, const int32_t *d_peak_baitID, const int32_t *d_peak_oeID,
                                            const double *d_scores, int64_t npeaks, int32_t ncols, int32_t ncond1, int32_t ncond2,
                                            int32_t merged, double score, double pvcut, double minDeltaAsinhScore, int64_t pair_capacity,
                                            int32_t *d_group_peak, int64_t *d_group_ptr, double *d_group_min_p, double *d_group_delta,
                                            int32_t *d_pair_row, int64_t *ngroups_host, int64_t *npairs_host);

/* The same call with the reference's `method` argument (method = c("min", "hmp"), chicdiff.R:2135-2137, 2146): how the pcol values of
 * a group's regions are combined.  d_group_min_p carries the combined p of the chosen method, and the filter (:2161) reads it.
 * CHICDIFF_CAND_MIN is the call above.  CHICDIFF_CAND_HMP is harmonicmeanp::p.hmp(pcol) as the reference calls it (no w, no L), for
 * a group of L regions with values p_1 .. p_L in the group's pair order:
 *   p'_k = 1 if p_k is NA or p_k > 1 (:2136), p_k otherwise
 *   x    = (sum_k 1 / p'_k) / L, the sum formed sequentially in pair order, each 1 / p'_k a correctly rounded division
 *   z    = (x - (log L + c)) / (pi / 2),   c = 1 + digamma(1) - log(2 / pi) = 0.874367040387922004
 *   hm_p = Q(z) = (1 / pi) int_0^inf exp(-t z - (2 / pi) t log t) sin(2 t) / t dt
 * Q is the upper tail of the Landau density of Wilson 2019 (PNAS 116:1195), eq. 4.  p_k = 0 gives x = inf and hm_p = 0; x >= 1, so
 * z > -14 for every L < 2^31; below z = -3.5 Q is 1 to double precision and the call returns exactly 1, never more.  A negative p
 * is outside the contract: it is not checked, and the arithmetic runs as written.  The value is pinned by the published formula,
 * evaluated with mpmath (tests/golden/landau_tail.json, and the paper's Table 1), and unpinned against the numerics of FMStable,
 * from which harmonicmeanp takes the Landau tail.  Any other method: CHICDIFF_E_INVALID. */
#define CHICDIFF_CAND_MIN 0
#define CHICDIFF_CAND_HMP 1
int chicdiff_hip_candidate_interactions_method_dev(chicdiff_hip_ctx *ctx, const int32_t *d_baitID, const int32_t *d_minOE,
                                                   const int32_t *d_maxOE, const double *d_p, int64_t n, const int32_t *d_peak_baitID,
                                                   const int32_t *d_peak_oeID, const double *d_scores, int64_t npeaks, int32_t ncols,
                                                   int32_t ncond1, int32_t ncond2, int32_t merged, double score, double pvcut,
                                                   double minDeltaAsinhScore, int32_t method, int64_t pair_capacity, int32_t *d_group_peak,
                                                   int64_t *d_group_ptr, double *d_group_min_p, double *d_group_delta, int32_t *d_pair_row,
                                                   int64_t *ngroups_host, int64_t *npairs_host);

/* limits of chicdiff_hip_control_draws_dev (below) */
#define CHICDIFF_CONTROL_MAX_CHR 1024     /* chromosome codes: the per-chromosome tables are kept per workgroup in LDS */
#define CHICDIFF_CONTROL_MAX_ATTEMPTS 256 /* redraws of one distance before the call gives up */
/* The draws of getControlRegionUniverse (chicdiff.R:430-481) from a 64-bit seed: as many control (baitID, oeID) pairs as RU has
 * non-empty regions, sorted, ready for chicdiff_hip_region_universe_dev (the expansion of :483-504 is that call, unchanged).  The
 * reference draws from R's unseeded stream; here the pairs are a pure function of (inputs, seed) — the same on every run, launch
 * shape and number of ranks.  The stream is this library's own, not R's: set.seed() is not reproduced.  Everything is enqueued on
 * the context's stream; the one host stop is the read of the counts.
 *
 * Random words: Philox4x32-10 (multipliers 0xD2511F53, 0xCD9E8D57, Weyl constants 0x9E3779B9, 0xBB67AE85), key = (seed & 0xffffffff,
 * seed >> 32), counter = (k & 0xffffffff, k >> 32, attempt, stream) for draw k = 0 .. n_regions - 1; (r0, r1, ..) = its output.
 *
 * Rules, by statement of the reference:
 *   n_regions (:466)          length(unique(RU$regionID)): the regions i with d_region_ptr[i + 1] > d_region_ptr[i].
 *   max_contact (:463-464)    max |baitID - otherEndID| over the RU rows whose bait lies on chromosome c.  A region's rows lie in
 *                             [minOE, maxOE] on one side of its bait (.expandAvoidBait, :353-367), so this is computed as
 *                             max(|bait - minOE|, |bait - maxOE|) over the non-empty regions, bait = d_ru_baitID[d_region_ptr[i]].  The
 *                             bait's chromosome is the one whose [chr_min, chr_max] holds it; an ID in no range is not on the map and
 *                             its rows drop out (the inner merge of :463).  d_max_contact[c] = 0: no contact.
 *   bait (:466-468)           stream 0, attempt 0: idx = high 64 bits of ((r0 | r1 << 32) * nb), bait = d_bmap_id[idx] (file order).  The
 *                             draw is DROPPED when d_bmap_chr[idx] is -1 (a name not on the map) or a chromosome without a contact:
 *                             merge(bmap[chr %in% max_contacts$chr], ..).  The control set may be smaller than the test set.
 *   std, min, max (:472-474)  max_contact[c] / 3.0 in double; chr_min[c], chr_max[c].
 *   distance (:434-444)       stream 1, attempts 0, 1, 2, ..: u = ((r0 >> 6) * 2^26 + (r1 >> 6) + 0.5) * 2^-52, exact, inside
 *                             [2^-53, 1 - 2^-53]; z = qnorm(u) by Wichura's AS 241 (PPND16); d = rint(z * std), ties to even (R's
 *                             round()); accepted when d != 0 and (bait + |d| < max or bait - |d| > min) — strict, as giveDists.
 *   seed of the region        fwd = bait + d; oeID = bait - d when fwd < min or fwd > max, else fwd — not strict, as giveOneSeed
 *   (:430-432)
 *   order (:480-481)          the kept pairs ascending by (baitID, oeID); regionID = 1 .. m by position.  Equal pairs are legal.
 *
 * Inputs: RU as chicdiff_hip_region_universe_dev left it — d_ru_baitID (int32[nru], rows in (regionID, otherEndID) order),
 * d_region_ptr (int64[n + 1]), d_minOE, d_maxOE (int32[n]); the baitmap d_bmap_id, d_bmap_chr (int32[nb], device; the chromosome as a
 * code of the restriction map, coded on the host); chr_min, chr_max (HOST, int32[nchr]): smallest and largest map ID per code
 * (min > max: a code without fragments).  The ranges must not overlap.
 * Outputs (device): d_ctrl_baitID, d_ctrl_oeID (int32, room for n, the first *m_host written); d_max_contact (int32[nchr]);
 * *n_regions_host, *m_host.
 * CHICDIFF_E_INVALID, with a message: n < 1 or nb < 1; nchr < 1 or nchr > CHICDIFF_CONTROL_MAX_CHR; overlapping ranges; a
 * d_region_ptr entry outside [0, nru] or descending; a bait of the baitmap with code >= nchr; no non-empty region; a distance still
 * rejected after CHICDIFF_CONTROL_MAX_ATTEMPTS attempts (the message names k, the bait and its chromosome code; the reference
 * would loop forever — only a chromosome that leaves a bait no valid distance gets there).  No chromosome with a contact, or every
 * draw dropped: CHICDIFF_OK with *m_host = 0. */
int chicdiff_hip_control_draws_dev(chicdiff_hip_ctx *ctx, const int32_t *d_ru_baitID, int64_t nru, const int64_t *d_region_ptr,
                                   const int32_t *d_minOE, const int32_t *d_maxOE, int64_t n, const int32_t *d_bmap_id,
                                   const int32_t *d_bmap_chr, int64_t nb, const int32_t *chr_min, const int32_t *chr_max, int32_t nchr,
                                   uint64_t seed, int32_t *d_ctrl_baitID, int32_t *d_ctrl_oeID, int32_t *d_max_contact,
                                   int64_t *n_regions_host, int64_t *m_host);

/* limits and status bits of chicdiff_hip_chicago_tables_dev (below) */
#define CHICDIFF_CHICAGO_MAX_PAIRS 1024          /* ntblb * ntlb */
#define CHICDIFF_CHICAGO_MAX_DISTBIN 1023        /* ndistbin (the NA code makes 1024 entries) */
#define CHICDIFF_CHICAGO_ROWS_PER_WORKGROUP 4096 /* consecutive rows a workgroup takes in each pass */
#define CHICDIFF_CHICAGO_NOT_A_FUNCTION 1        /* bits of *status_host */
#define CHICDIFF_CHICAGO_BAD_CODE 2
/* The Chicago background tables of ONE replicate (chicdiff.R:656-692 the per-fragment and per-pair tables, 538-548 the input of
 * .chicEstimateDistFun) from the columns of chicagoData@x, rows r = 0 .. nrows - 1 in ANY order.  No sort.
 * WINNER RULE: every "first" of the reference follows setkey(x, baitID, otherEndID), a stable sort, and drop_duplicates / unique
 * keeping the first row, so it is the row that minimises (baitID, otherEndID, r) within its group:
 *   per bait b       d_sj[b - id_min] = s_j, d_tblb_of[b - id_min] = tblb of the winner among the rows with baitID = b    (:659)
 *   per other end o  d_si, d_tlb_of likewise among the rows with otherEndID = o                                            (:668)
 *                    the winner's values are kept even when they are NA; IDs outside [id_min, id_min + nid) are ignored; an
 *                    ID that no row shows stays NaN / -1
 *   per (tblb, tlb)  d_T[tblb * ntlb + tlb] = Tmean of the winner among the rows whose two codes are both non-NA (IDs are not
 *                    filtered here); a pair that no row shows stays NaN                                                    (:678-681)
 *   per distbin d    d_ref[d] = the refBinMean of the rows with that code and a non-NA refBinMean (an NA distbin is a value of its
 *                    own: the last entry, d_ref[ndistbin]); NaN = no such row.  The non-NaN entries are the multiset .chicEstimateDistFun
 *                    sorts and fits (:543-548) exactly when refBinMean is a function of distbin, as Chicago's is.  A code with
 *                    two different values gets NaN and sets CHICDIFF_CHICAGO_NOT_A_FUNCTION in *status_host (the call still
 *                    returns CHICDIFF_OK: the caller builds that replicate's distance function on the host)
 * All of these are minima of integers: the result does not depend on the order of the rows, and equals the host twin
 * (chicdiff_amd.pipeline.background_tables) bit for bit.
 * Inputs, device, nrows entries each: d_bait, d_oe (int32); d_s_j, d_s_i, d_Tmean, d_refBinMean (double, NaN = NA); d_tblb, d_tlb,
 * d_distbin (int32 level codes in [0, ntblb) / [0, ntlb) / [0, ndistbin), -1 = NA).  Outputs, device, filled with NaN / -1 by
 * the call itself: d_sj, d_si (double), d_tblb_of, d_tlb_of (int32) [nid] — row s of the (S, nid) tables
 * chicdiff_hip_fragment_background_dev takes; d_T [ntblb * ntlb]; d_ref [ndistbin + 1].
 * CHICDIFF_E_INVALID, with a message: nrows < 1 or nrows >= 2^32 (the row index is half of a 64-bit atomic word); nid < 1;
 * ntblb < 1, ntlb < 1 or ntblb * ntlb > CHICDIFF_CHICAGO_MAX_PAIRS, ndistbin < 0 or ndistbin > CHICDIFF_CHICAGO_MAX_DISTBIN (both
 * tables are kept per workgroup in LDS); a code outside its range (nothing of the outputs is to be used then).
 * chicdiff_hip_chicago_tables_caps: the three constants below, as the library was built (any pointer may be NULL). */
int chicdiff_hip_chicago_tables_dev(chicdiff_hip_ctx *ctx, const int32_t *d_bait, const int32_t *d_oe, const double *d_s_j,
                                    const double *d_s_i, const double *d_Tmean, const double *d_refBinMean, const int32_t *d_tblb,
                                    const int32_t *d_tlb, const int32_t *d_distbin, int64_t nrows, int32_t id_min, int32_t nid,
                                    int32_t ntblb, int32_t ntlb, int32_t ndistbin, double *d_sj, double *d_si, int32_t *d_tblb_of,
                                    int32_t *d_tlb_of, double *d_T, double *d_ref, int32_t *status_host);
int chicdiff_hip_chicago_tables_caps(int32_t *max_pairs, int32_t *max_distbin, int32_t *rows_per_workgroup);

/* limits of chicdiff_hip_countput_dev (below) */
#define CHICDIFF_COUNTPUT_MAX_REP 64                     /* replicates of one condition: their row offsets are kept per workgroup in LDS */
#define CHICDIFF_COUNTPUT_KEY_ROWS_PER_WORKGROUP 1024    /* consecutive rows a workgroup of the key pass takes */
#define CHICDIFF_COUNTPUT_REDUCE_ROWS_PER_WORKGROUP 256  /* consecutive sorted positions a workgroup of the heads / reduce passes takes */
/* countput of ONE condition (chicdiff.R:708-735 the rows kept per replicate, :754-768 the aggregation): per observed (baitID,
 * otherEndID) pair the mean N, the mean Bmean, the largest score and the other end's midpoint — what plotDiffBaits() draws.  Equal,
 * bit for bit and in row order, to the host twin (chicdiff_amd.pipeline._countput, a pandas groupby); the rule, stated in full:
 *
 * Take the condition's replicates in the order given and concatenate their rows: global row index g, replicate 0's rows first, each
 * replicate in its own row order.
 *   rows kept    a row is kept when its distSign is not NaN (:715) AND its otherEndID is on the map, that is inside
 *                [id_min, id_min + nid) with d_chr[otherEndID - id_min] >= 0 (the inner merge with the map, :724).  baitID is NOT
 *                filtered.
 *   groups       kept rows with equal (baitID, otherEndID) form a group, within and across replicates (a pair repeated inside one
 *                replicate is legal and joins the same group).
 *   Nav, Bav     over the group's rows in ascending g; Nav from N (int32 converted to double, never NA), Bav from Bmean.  A NaN value
 *                is skipped; otherwise
 *                    cnt += 1;  y = v - c;  t = s + y;  c = (t - s) - y;  if (c != c) c = 0;  s = t          (s = c = 0 at the start)
 *                and the result is s / cnt, NaN when cnt = 0: a Kahan sum in row order, divided once.  Plain fp64, no reassociation,
 *                no contraction.  The reset of c is what keeps [inf, 1, 2] at inf (c would be NaN from the second row on).
 *   score        NaN is skipped; the first non-NaN value starts the maximum, and a later value replaces it only when it is STRICTLY
 *                greater: of 0.0 and -0.0 the earlier one stays.  NaN when the group has no value.
 *   oeID_mid     (start + end) / 2 of the other end = d_midsum[otherEndID - id_min] / 2.0, exact.
 *   order        groups are ordered by the smallest g in them (first appearance) — the twin's order (groupby(sort = False)).  The
 *                reference's own order differs: its merge(x, rmap_copy, by = "otherEndID") re-keys each replicate by otherEndID before
 *                the rows are stacked.  Nothing downstream reads the order (plotDiffBaits subsets by bait).
 * mean and max follow the twin, which is the project's statement of this stage: R's mean() carries a NA through and its max() has no
 * na.rm here; both are kept as the twin has them.
 *
 * Inputs: nrep replicates; d_bait, d_oe, d_N, d_Bmean, d_score, d_distSign are HOST arrays of nrep entries with device pointers
 * inside (as the key tables of chicdiff_hip_count_join_multi_dev): int32 baitID, otherEndID, N and double Bmean, score, distSign (NaN =
 * NA), nrows[r] entries each (nrows: HOST, int64[nrep]; a replicate with 0 rows is valid and its pointers are not read).  The map:
 * id_min, nid, d_midsum (int64[nid]), d_chr (int32[nid], -1 = not on the map).
 * Outputs (device), room for sum(nrows) entries each, the first *ngroups_host written: d_out_bait, d_out_oe (int32), d_Nav, d_Bav,
 * d_out_score, d_mid (double).  They may be NULL when sum(nrows) = 0.
 * No value passes through an atomic; launch shape, workgroup size and arrival order do not show in any bit.  Everything is enqueued
 * on the context's stream; the one host stop is the read of the count.
 * CHICDIFF_E_INVALID, the message naming the limit: nrep < 1 or nrep > CHICDIFF_COUNTPUT_MAX_REP; nid < 1; id_min + nid > INT32_MAX
 * (a map ID of INT32_MAX: the all-ones sort key marks a dropped row); a negative nrows[r]; sum(nrows) >= 2^31 (g is a 32-bit sort
 * value).  sum(nrows) = 0 and every row dropped: CHICDIFF_OK with *ngroups_host = 0.
 * chicdiff_hip_countput_caps: the three constants above, as the library was built (any pointer may be NULL). */
int chicdiff_hip_countput_dev(chicdiff_hip_ctx *ctx, int32_t nrep, const int32_t *const *d_bait, const int32_t *const *d_oe,
                              const int32_t *const *d_N, const double *const *d_Bmean, const double *const *d_score,
                              const double *const *d_distSign, const int64_t *nrows, int32_t id_min, int32_t nid,
                              const int64_t *d_midsum, const int32_t *d_chr, int32_t *d_out_bait, int32_t *d_out_oe, double *d_Nav,
                              double *d_Bav, double *d_out_score, double *d_mid, int64_t *ngroups_host);
int chicdiff_hip_countput_caps(int32_t *max_rep, int32_t *key_rows_per_workgroup, int32_t *reduce_rows_per_workgroup);

/* limits of chicdiff_hip_table_text_dev / chicdiff_hip_table_write_dev (below) */
#define CHICDIFF_TABLE_MAX_COLUMNS 64          /* columns of a table: their descriptors travel as one kernel argument */
#define CHICDIFF_TABLE_MAX_DICT 4096           /* entries of one dictionary column */
#define CHICDIFF_TABLE_MAX_ENTRY_BYTES 4096    /* bytes of one dictionary entry */
#define CHICDIFF_TABLE_ROWS_PER_TILE 256       /* consecutive rows a workgroup takes in both passes: one row per lane */
#define CHICDIFF_TABLE_LDS_BYTES 65536         /* text of a tile staged in LDS at a time; a tile with more goes through it in chunks */
#define CHICDIFF_TABLE_MAX_CELL_BYTES 24       /* the longest number: -2.2250738585072014e-308 */
#define CHICDIFF_COL_INT32 0
#define CHICDIFF_COL_INT64 1
#define CHICDIFF_COL_FLOAT64 2
#define CHICDIFF_COL_DICT 3
/* A table of device columns written as text: what pandas' DataFrame.to_csv(index = False) writes for the same frame (pandas 2.x, no
 * float_format, no quoting needed), byte for byte — the writing of _countput.csv and _results.csv (chicdiff_amd.pipeline; the
 * reference saves .Rds, chicdiff.R:769, :2062).  The rule, stated in full (tests/table_text_twin.py is the same in plain Python):
 *   - a table is ncol >= 2 columns of n rows and one separator byte (a tab, a comma or a blank); row r is its cells joined by the
 *     separator, followed by '\n'.  One-column tables are not offered: pandas writes a NaN of a one-column frame as "".
 *   - CHICDIFF_COL_INT32 / _INT64: the decimal digits, '-' in front of a negative value.
 *   - CHICDIFF_COL_FLOAT64: NaN of any sign or payload gives no byte; +inf gives inf, -inf gives -inf; every other value gives Python's
 *     repr(float): digits d1 .. dk (k <= 17), the shortest string that reads back to the value and among the shortest the one closest
 *     to it; with decpt the position of the decimal point (value = 0.d1 .. dk * 10^decpt), -4 < decpt <= 16 gives the positional
 *     form, which always has a fractional part (5.0, -0.0, 0.0001, 9999999999999998.0); any other decpt gives d[.ddd]e+XX / e-XX
 *     with at least two exponent digits (1e+16, 1e-05, 5e-324).  A cell is at most CHICDIFF_TABLE_MAX_CELL_BYTES bytes.
 *     (chicdiff_amd/csrc/table_text.h decides this with integers alone: 64 x 128-bit products against pow10_table.h.)
 *   - CHICDIFF_COL_DICT: each row carries an int32 code into a table of at most CHICDIFF_TABLE_MAX_DICT byte strings (dict_off[ndict
 *     + 1] ascending from 0, dict_bytes: HOST memory, copied by the call); a negative code gives no byte, as pandas writes None / NaN
 *     in an object column; d_data = NULL means entry 0 for every row (a constant column).  An entry that holds the separator, '"',
 *     '\r' or '\n' is refused: pandas would quote it.  A code >= ndict is refused once met (nothing is read out of bounds).
 * Two passes (table_text_kernels.hip): a length pass, one lane per row, leaves every row's byte count and every tile's total; one scan
 * of the tile totals places the tiles and gives the size (the first host stop); the write pass scans the row lengths inside the
 * workgroup, formats every row into LDS at its offset and stores the tile's bytes as one contiguous run.  Placement comes from the two
 * scans alone and no value passes through an atomic: the bytes are a function of the inputs, not of launch shape or arrival order.
 * Limits, each refused by name with CHICDIFF_E_INVALID: ncol < 2 or > CHICDIFF_TABLE_MAX_COLUMNS; n < 0 or >= 2^31; an unknown
 * kind; a NULL column with n > 0 (other than a dictionary's codes); a dictionary with no or too many entries, with offsets that do
 * not ascend from 0, with an entry over CHICDIFF_TABLE_MAX_ENTRY_BYTES or one that needs quoting; a text of 2^40 bytes or more.
 *
 * chicdiff_hip_table_check: the refusals above on their own (host only, no context; d_data is compared with NULL, never read); the
 * message goes to err[errcap].
 * chicdiff_hip_table_text_dev: the device stage alone.  d_out[cap] is the caller's device buffer; *nbytes_host = the size of the text.
 * cap < that size: nothing is written and the call returns CHICDIFF_OK — call again with room (cap = 0, d_out = NULL asks for the size).
 * chicdiff_hip_table_write_dev: the text into a file.  The header bytes (header_bytes >= 0, written as they are — the caller ends
 * them with '\n') go first unless `append` is set; append = 1 adds the rows behind what the file holds (created if missing).  The text
 * is formed in a grow-only buffer of the context and leaves through the two halves of the bounded pinned area of
 * chicdiff_hip_chinput_read_dev (2 x 64 MiB at most, never file-sized): host_copy_threads threads pwrite one half while the DMA of
 * the other runs.  A failed open, write or close fails the call with CHICDIFF_E_INVALID, the message naming the path and the system's
 * reason; the file is then removed if this call created it.  *written_host (may be NULL) = bytes written, header included.
 * Timers (chicdiff_hip_kernel_times): table_len, table_scan, table_write, table_download (the DMAs and the file writes between them).
 * chicdiff_hip_table_text_caps: rows per tile, LDS bytes, most columns, most dictionary entries (any pointer may be NULL). */
typedef struct {
    int32_t kind;              /* CHICDIFF_COL_* */
    int32_t ndict;             /* CHICDIFF_COL_DICT: entries, 1 .. CHICDIFF_TABLE_MAX_DICT; otherwise ignored */
    const void *d_data;        /* DEVICE: n values (int32 / int64 / float64), or n int32 codes, or NULL (dictionary: entry 0 throughout) */
    const int32_t *dict_off;   /* HOST: ndict + 1 offsets */
    const uint8_t *dict_bytes; /* HOST: the entries' bytes */
} chicdiff_table_column;
int chicdiff_hip_table_check(const chicdiff_table_column *cols, int32_t ncol, int64_t n, int32_t sep, char *err, int32_t errcap);
int chicdiff_hip_table_text_dev(chicdiff_hip_ctx *ctx, const chicdiff_table_column *cols, int32_t ncol, int64_t n, int32_t sep,
                                uint8_t *d_out, int64_t cap, int64_t *nbytes_host);
int chicdiff_hip_table_write_dev(chicdiff_hip_ctx *ctx, const char *path, int32_t append, const uint8_t *header, int64_t header_bytes,
                                 const chicdiff_table_column *cols, int32_t ncol, int64_t n, int32_t sep, int64_t *written_host);
int chicdiff_hip_table_text_caps(int32_t *rows_per_tile, int32_t *lds_bytes, int32_t *max_columns, int32_t *max_dict);
/* The double -> text function of the rule on its own: text (24 n bytes, slot i = bytes 24 i .., zero-filled behind the cell) and len
 * (n).  _dev: through the device function, d_x / d_text / d_len device memory; the other: the same function compiled for the host, no
 * device and no context (machines without a GPU check the rule with it). */
int chicdiff_hip_selftest_format_double_dev(chicdiff_hip_ctx *ctx, const double *d_x, int64_t n, uint8_t *d_text, int32_t *d_len);
int chicdiff_hip_selftest_format_double(const double *x, int64_t n, uint8_t *text, int32_t *len);

/* a6 + a7 — estimateDispersions + nbinomWaldTest (chicdiff.R:1573-1574, 1602-1603, 1643-1644,
 * 1673-1674) for design ~condition (group[j] in {0,1}, both present) or ~1 (all group[j]==0).
 * d_nf = normalizationFactors (n x S).  `group` is a HOST array of S ints. */
int chicdiff_hip_nbglm_fit_dev(chicdiff_hip_ctx *ctx, const int32_t *d_counts, const double *d_nf, int64_t n,
                               int32_t S, const int32_t *group, const chicdiff_nbglm_opts *opts,
                               const chicdiff_nbglm_out *d_out, chicdiff_nbglm_scalars *scalars);

/* Same, HOST buffers in and out (what the R .Call shim passes: INTEGER(counts), REAL(nf)). */
int chicdiff_hip_nbglm_fit(chicdiff_hip_ctx *ctx, const int32_t *counts, const double *nf, int64_t n, int32_t S,
                           const int32_t *group, const chicdiff_nbglm_opts *opts, const chicdiff_nbglm_out *out,
                           chicdiff_nbglm_scalars *scalars);

/* a5 + a4 + a6 + a7 in one call — size factors -> sc(theta) -> dispersions -> Wald test
 * (chicdiff.R:1561-1562, 1666-1674), with size factors and offsets kept in HBM.  theta = NaN uses
 * normFactorsM3 (norm = "fullmean"); d_fullMean = NULL uses the size factors alone (norm = "standard",
 * chicdiff.R:1572-1575).  sf_host (S doubles) may be NULL. */
int chicdiff_hip_wald_test_dev(chicdiff_hip_ctx *ctx, const int32_t *d_counts, const double *d_fullMean, int64_t n,
                               int32_t S, const int32_t *group, double theta, const chicdiff_nbglm_opts *opts,
                               const chicdiff_nbglm_out *d_out, chicdiff_nbglm_scalars *scalars, double *sf_host);

/* a8 — theta grid (chicdiff.R:1619-1662): for each theta, sc(theta) -> design ~1 fit ->
 * deviances[t] = sum(deviance).  d_fullMean n x S, sf_host the null size factors. */
int chicdiff_hip_theta_grid_dev(chicdiff_hip_ctx *ctx, const int32_t *d_counts, const double *d_fullMean,
                                const double *sf_host, int64_t n, int32_t S, const double *thetas,
                                int32_t ntheta, const chicdiff_nbglm_opts *opts, double *deviances_host);

/* Wald p-values alone: p[i] = 2*pnorm(-|stat[i]|) (Cody's algorithm, the one R's pnorm uses). */
int chicdiff_hip_wald_pvalues_dev(chicdiff_hip_ctx *ctx, const double *d_stat, int64_t n, double *d_p);

/* Device-math self test: out[i] = f(x[i]) with op 0 log (polynomial), 1 log (table), 2 reciprocal,
 * 3 lgamma, 4 digamma, 5 2*pnorm(-|x|), 8 exp (table) — the special functions the fit kernels are built on —, 9 qnorm (AS 241
 * with the polynomial log in its tails, 0 < x < 1), as chicdiff_hip_control_draws_dev calls it. */
int chicdiff_hip_selftest_math_dev(chicdiff_hip_ctx *ctx, int32_t op, const double *d_x, int64_t n, double *d_out);
/* out[i] = Q(z[i]), the Landau tail of CHICDIFF_CAND_HMP, as the overlap kernel of chicdiff_hip_candidate_interactions_method_dev
 * calls it: 1 for z <= -3.5, 0 for +inf, NaN for NaN. */
int chicdiff_hip_selftest_landau_dev(chicdiff_hip_ctx *ctx, const double *d_z, int64_t n, double *d_out);
/* The same for the functions of two arguments / two results that carry the dispersion objective, the constant part of the NB
 * log-likelihood and the reported deviance, each called as the kernels call it; y[i] is an integer count held in a double:
 * op 10 lgr_eval_t(lgr_make_t(x), y) and 11 lgr_eval(lgr_make(x), y) = lgamma(y + x) - lgamma(x), 12 lgr_eval(lgr_one(), y) = log(y!),
 * 13 tlog1p_from(x, 1 + x, rcp(1 + x)) and 14 flog1p_from(...) = log1p(x), 15 rcp_or_div(x) = 1 / x, 16 stirling(x, log x, 1 / x):
 * out = lgamma(x), out2 = digamma(x) for x >= 10, 17 rlog_t(x) = R's log(x), 18 the host's table of log(y!), y < 1024.
 * out2 is NaN for the ops with one result. */
int chicdiff_hip_selftest_math3_dev(chicdiff_hip_ctx *ctx, int32_t op, const double *d_x, const double *d_y, int64_t n, double *d_out,
                                    double *d_out2);
/* The dispersion objective on its own: log posterior of log(alpha) (DESeq2 fitDisp's log_posterior), its derivative and alpha =
 * exp(log alpha) at K points per row, d_log_alpha[i * K + k], computed by the functions the line searches and the grid fallback
 * stop on, from the row records the fit's first kernel writes.  counts / nf / group / opts as for chicdiff_hip_nbglm_fit_dev.
 * d_prior_mean: per row, or NULL for the gene-wise objective (no prior); prior_var: the prior's variance.  live_rows = 0: one row per
 * lane; 1 .. 64: that many rows per wave, their samples spread across lanes as the line search does for so many live rows at the end
 * of a launch (CHICDIFF_E_INVALID where it would not) — *lanes_per_row (may be NULL) gets the lanes a row was given (1: row per lane).
 * Results: d_lp, d_dlp, d_alpha (n x K) and d_mu (n x S, column-major): the means max(nf * group mean, minmu) the evaluations used.
 * An all-zero row has no objective: NaN everywhere. */
int chicdiff_hip_selftest_objective_dev(chicdiff_hip_ctx *ctx, const int32_t *d_counts, const double *d_nf, int64_t n, int32_t S,
                                        const int32_t *group, const chicdiff_nbglm_opts *opts, const double *d_log_alpha, int32_t K,
                                        const double *d_prior_mean, double prior_var, int32_t live_rows, double *d_lp, double *d_dlp,
                                        double *d_alpha, double *d_mu, int32_t *lanes_per_row);

/* TEST ENTRY, not a product path.  The global stage of a fit — what lies between the gene-wise search and the MAP search: the trend
 * (parametric, opts->fitType = 1 mean, 2 local, or opts->trendCoef given), the log residuals, their median and MAD, and the prior
 * variance (closed form, opts->dispPriorVar given, or by simulation for S - p <= 3) — on the caller's device columns baseMean,
 * dispGeneEst (NaN in all-zero rows) and allZero (n rows) instead of the columns the gene-wise search left.  The fit's own function
 * runs on them, and a parametric trend that fails is answered as a fit answers it (option "local_trend_substitute").  Single rank only.
 * Results: d_dispFit (n; the stage itself forms the column under a local trend only: NaN otherwise, and in all-zero rows),
 * d_resid (n; NaN where dispGeneEst < 100 minDisp or the row is all zero), hist40 (HOST, 40: the counts the simulated prior was
 * matched to; zero when the prior is not found by simulation), the local trend's vertices in ascending x (HOST: *lf_nv, and lf_x,
 * lf_h, lf_f, lf_d of 100 doubles each: position, bandwidth, value, slope; *lf_nv = 0 without a local trend), and scalars:
 * trendCoef, varLogDispEsts, dispPriorVar, trendOuterIter and the status bits CHICDIFF_ST_TREND_FAILED / _TREND_LOCAL / _PRIORVAR_MC
 * (sumDeviance NaN, nAllZero 0: not of this stage).  A mean trend without a usable row: CHICDIFF_E_NUMERIC, as in a fit. */
int chicdiff_hip_selftest_global_stage_dev(chicdiff_hip_ctx *ctx, const double *d_baseMean, const double *d_dispGeneEst,
                                           const int32_t *d_allZero, int64_t n, int32_t S, int32_t p, const chicdiff_nbglm_opts *opts,
                                           double *d_dispFit, double *d_resid, double *hist40, int32_t *lf_nv, double *lf_x, double *lf_h,
                                           double *lf_f, double *lf_d, chicdiff_nbglm_scalars *scalars);
/* TEST ENTRY.  hist40 (HOST, 40) = the counts of hist(x[x > -10 & x < 10], breaks = -20:20/2) over the device column d_resid (n; NaN =
 * no residual), by the kernel the simulated prior counts its residuals with. */
int chicdiff_hip_selftest_resid_hist_dev(chicdiff_hip_ctx *ctx, const double *d_resid, int64_t n, double *hist40);

/* Host-side self tests of the pieces behind CHICDIFF_ST_PRIORVAR_MC (no device, no context).
 * _r_random: set.seed(seed) followed by n draws of kind 0 runif(n), 1 rnorm(n), 2 rexp(n), 3 rgamma(n, shape = a,
 * scale = b) from R's default generators (Mersenne-Twister, inversion).
 * _prior_mc: DESeq2 estimateDispersionsPriorVar for residual d.f. df in 1..3: dens_out (200 x 40, row-major, may be
 * NULL) = the densities of its 200 simulated residual distributions; *prior_var_out (may be NULL) = the prior
 * variance matched to hist40, the counts of hist(residuals, breaks = -20:20/2). */
/* _chinput: the parser behind chicdiff_hip_chinput_read on its own: the three columns of up to `cap` rows, *nrows = rows in
 * the file; on a parse error the message goes to err[errcap]. */
int chicdiff_hip_selftest_chinput(const char *path, int32_t nthreads, int64_t cap, int32_t *bait, int32_t *oe, int32_t *N,
                                  int64_t *nrows, char *err, int32_t errcap);
/* _peaks (host only, no context): a single-threaded host statement of the peak-matrix rule above — the same header function, strtod
 * for the decimals, the same filter — so that the rule can be checked where there is no GPU.  A test entry, not a product path.
 * targets / cond_of_target[ntargets]: the targetColumns and the condition of each; ints (6, cap), dist (cap), scores (nscore, cap),
 * line_off (cap), kept_idx (cap), filtered (cap), score_target (ntargets): any may be NULL; info: the words above.  A header or
 * malformed-row error: CHICDIFF_E_INVALID, the message in err[errcap]. */
int chicdiff_hip_selftest_peaks(const char *path, const char *const *targets, int32_t ntargets, double score, const int32_t *cond_of_target,
                                int32_t ncond, int32_t replicate_rule, int64_t cap, int32_t *ints, double *dist, double *scores,
                                int64_t *line_off, int64_t *kept_idx, int32_t *filtered, int32_t *score_target, int64_t *info, char *err,
                                int32_t errcap);
int chicdiff_hip_selftest_r_random(int32_t kind, uint32_t seed, double a, double b, int64_t n, double *out);
int chicdiff_hip_selftest_prior_mc(int32_t df, const double *hist40, double *dens_out, double *prior_var_out);
/* _sched_class (host only): the class the gene-wise line search's schedule ("line_search_schedule" = mode, 1 .. 4) puts a row in,
 * from its start value alpha_init and its smaller group mean — cls_out[n], lower = visited earlier; bounds[7] (may be NULL): the
 * first class that goes through the queue when 0 .. 6 of the half-decade classes are dealt out statically. */
int chicdiff_hip_selftest_sched_class(int32_t mode, double min_disp, const double *alpha_init, const double *group_mean, int64_t n,
                                      int32_t *cls_out, int32_t *bounds);
/* _queue_claim (host only): the claim rule of the gene-wise line search's two-ended queue, as the kernel applies it.  `old` is the
 * queue word before the claim (claims from the head in its low half, from the end in its high half).  Returns 1 if a claim that found
 * `old` is valid, 0 if not, and the chunk it names in *chunk_out; *again_out (may be NULL): whether a filler wave whose claim found
 * `old` (claimed != 0; claimed == 0: a filler that has not claimed yet) may claim once more, given the first chunk that lies wholly
 * in the rows fillers may take (first_back; >= chunks: none) and the stop share in percent ("line_search_filler_stop"). */
int chicdiff_hip_selftest_queue_claim(uint64_t old, int32_t back, uint32_t chunks, uint32_t first_back, int32_t stop_percent, int32_t claimed,
                                      uint32_t *chunk_out, int32_t *again_out);
/* _trend_exchange (host only): the words in which the single-launch trend kernel's workgroups hand each other a pass's partial sums
 * ("trend_exchange"), as the kernel forms and accepts them.  op 0: words[2 i], words[2 i + 1] = x[i] packed under `tag` (pass + 1), i < n;
 * op 1: x[i] = the double in words[2 i], words[2 i + 1], and accept[i] (may be NULL) = whether a reader of `tag` takes both words;
 * op 2: accept[k] = whether a reader of `tag` takes words[k], k < n.  Tag 0 (never written) is taken by nobody. */
int chicdiff_hip_selftest_trend_exchange(int32_t op, uint32_t tag, int64_t n, double *x, uint64_t *words, int32_t *accept);
/* _sf_bin (host only): the value bins of the single-rank size-factor select, as its kernels apply them.  *nbins_out (may be NULL): the
 * number of bins per column for S samples (<= 16); bin_out[n]: the bin of each key x (log count - row log geometric mean); sub_out[n] (may be NULL):
 * its sub-bin inside bin `sub_of`.  Both never decrease as x grows: all the select's exactness asks of them. */
int chicdiff_hip_selftest_sf_bin(int32_t S, const double *x, int64_t n, int32_t *nbins_out, int32_t *bin_out, int32_t sub_of, int32_t *sub_out);
/* _ihw_knots_dev: the knots of every (fold, group) of chicdiff_hip_ihw_train_dev's step 4, as the device finds them with chunks of
 * `chunk_len` rows (0 = the default, else one of chicdiff_hip_ihw_caps' list), as CSR on the HOST: entry q = f * nbins + (g - 1) owns
 * x_host / c_host [ptr_host[q] .. ptr_host[q + 1]).  *nbins_host = the groups used, *nknots_host = the knots in all.  Two calls: with
 * cap = 0 only the two counts are written; else ptr_host needs nfolds * nbins + 1 entries and x_host, c_host `cap` >= *nknots_host. */
int chicdiff_hip_selftest_ihw_knots_dev(chicdiff_hip_ctx *ctx, const double *d_pvalue, const double *d_covariate, int64_t n, int32_t nbins,
                                        int32_t nfolds, uint64_t seed, int32_t chunk_len, int64_t cap, int64_t *ptr_host, double *x_host,
                                        int32_t *c_host, int32_t *nbins_host, int64_t *nknots_host);
/* _ihw_orient (host only, no context): step 4's exact knot test as compiled for the host, on n triples of points (x in [0, 1], count
 * below 2^31): sign[i] = +1 when b lies strictly above the chord from a to c (a knot), 0 when the three are collinear, -1 below. */
int chicdiff_hip_selftest_ihw_orient(const double *ax, const int32_t *ac, const double *bx, const int32_t *bc, const double *cx,
                                     const int32_t *cc, int64_t n, int32_t *sign);

/* Timing of the last *_dev call's kernels, measured with HIP events on the context's stream:
 * fills up to `cap` (name, milliseconds, launches) records; returns the number available. */
typedef struct {
    const char *name;
    double ms;
    int32_t launches;
    int32_t _pad;
    double bytes; /* "allreduce" / "allgather" (timing mode 1): payload this rank handed to the transport; 0 for kernels */
} chicdiff_kernel_time;
int32_t chicdiff_hip_kernel_times(chicdiff_hip_ctx *ctx, chicdiff_kernel_time *out, int32_t cap);
/* on: 0 = off, 1 = every stage of a call gets an event pair, 2 = only the three fit kernels (disp_gene, disp_map, wald_irls),
 * 3 = the gene-wise line search alone: an event pair is a packet pair on the stream — ~12 us of a 1.3 ms fit per bracketed
 * stage, 0.09 ms per fit with all ~20 stages bracketed */
int chicdiff_hip_enable_timing(chicdiff_hip_ctx *ctx, int32_t on);

#ifdef __cplusplus
}
#endif
#endif
