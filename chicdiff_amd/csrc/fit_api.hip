// fit_api.hip — the launch sequence of one fit.  Everything is enqueued on one HIP stream.  On a single rank the host blocks once, to
// read the fit's scalars back at the end; sharded, it also looks at the trend's `finished` flag once per
// batch of IRLS passes and at the verdict of each median's candidate gather.  With world_size > 1
// every global sum goes through a sum-all-reduce on the same stream: the library's own RCCL
// communicator (chicdiff_hip_rccl_init) or the caller's callback (chicdiff_hip_set_allreduce).
#include <thread>

#include "ctx.h"

double *cd::resid_hist_of(const FitWork &w) { return sums_of(w) + 32; }

// ---- HIP backend of fit_driver.h -----------------------------------------------------------
struct HipBackend {
    chicdiff_hip_ctx *c;
    FitDims d;
    Opts o;
    SelArgs sa;  // key source of the running select
    int err = 0;
    bool local = false;  // a sharded fit whose rows are all on this rank for this step (MAD over the gathered trend rows): single-rank path
    bool all_rounds = false;  // this pass of the call takes every histogram round (option "select_all_rounds", or the retry after an overflow)
    bool sharded() const { return c->allreduce && !local; }
    int world() const { return sharded() ? (c->world > 1 ? c->world : 2) : 1; }  // callback set => sharded protocol
    int allreduce(double *buf, int64_t n) { return sharded() ? do_allreduce(c, buf, n) : 0; }
    double *sums() { return c->w.partials; }  // sharded: the per-block partials themselves are all-reduced (one launch fewer per pass)
    int64_t sums_len() const { return (int64_t)trend_blocks() * kTrendSums; }
    double *hist() { return c->w.hist; }
    void trend_init() { launch_trend_init(d, c->w, o, c->stream); }
    void trend_pass(bool fused) {
        Scope t(c, "trend_pass");
        launch_trend_pass(d, c->w, o, c->stream, fused);
    }
    void trend_step() { launch_trend_step(d, c->w, o, c->stream); }
    const FitScalars *sync_scalars() {
        hipError_t e = hipMemcpyAsync(c->h_sc, c->w.sc, sizeof(FitScalars), hipMemcpyDeviceToHost, c->stream);
        if (e == hipSuccess) e = hipStreamSynchronize(c->stream);
        if (e != hipSuccess) {
            err = fail(c, CHICDIFF_E_HIP, "reading fit scalars: %s", hipGetErrorString(e));
            c->h_sc->finished = 1;  // stop the driver; the caller sees `err`
        }
        return c->h_sc;
    }
    void sel_hist(const SelSpec &, int shift) {
        Scope t(c, "select_hist");
        sa.shift = shift;
        launch_sel_hist(sa, c->w, c->stream);
    }
    void sel_step(const SelSpec &, int shift) {
        Scope t(c, "select_step");
        sa.shift = shift;
        launch_sel_step(sa, c->w, c->stream);
    }
    bool sel_shortcut(const SelSpec &) {
        if (sharded() || all_rounds) return false;  // sharded: candidates live on other ranks too
        Scope t(c, "select_shortcut");
        sa.shift = 40;
        launch_sel_shortcut(sa, c->w, c->stream);
        finished_by_shortcut = true;  // its last kernel also did what sel_finish does
        return true;
    }
    bool finished_by_shortcut = false;
    void sel_finish(const SelSpec &) {
        if (!finished_by_shortcut) launch_sel_finish(sa, c->w, c->stream);
    }
    // sharded shortcut
    int world_size() const { return c->world; }
    bool sel_can_gather() const { return c->world <= kSelMaxWorld && !all_rounds; }
    double *sel_counts() { return c->w.selcnt; }
    void sel_keep_local_hist(const SelSpec &) { launch_sel_keep_local(sa, c->w, c->stream); }
    void sel_gather_counts(const SelSpec &) { launch_sel_gather_counts(sa, c->w, c->world, c->rank, c->stream); }
    void sel_gather_place(const SelSpec &) {
        Scope t(c, "select_gather");
        sa.shift = 40;
        launch_sel_gather_place(sa, c->w, c->world, c->rank, c->stream);
    }
    void sel_gather_finish(const SelSpec &) { launch_sel_gather_finish(sa, c->w, c->world, c->rank, c->stream); }
    // no look at the device: a list that did not fit sets FitScalars::sel_overflow, which the host sees at the call's last
    // synchronisation and answers with a refit over every histogram round (every rank takes the same decision)
    bool sel_gather_done() { return true; }
};

// exact medians by radix select; results land in w.sc (see sel_finish_kernel)
static int run_select(chicdiff_hip_ctx *c, SelArgs a, bool all_rounds, bool local = false) {
    HipBackend be{c, FitDims{}, Opts{}, a};
    be.local = local;
    be.all_rounds = all_rounds;
    SelSpec spec{a.mode, a.ncol};
    const int rc = drive_select(be, spec);
    if (rc) return c->err[0] ? CHICDIFF_E_COMM : fail(c, CHICDIFF_E_COMM, "select: all-reduce failed");
    return CHICDIFF_OK;
}

int cd::check_counts_group(chicdiff_hip_ctx *c, int64_t n, int32_t S, const int32_t *group, FitDims &d) {
    if (n < 1 || n > 2147483647ll || S < 2 || S > kMaxS)
        return fail(c, CHICDIFF_E_INVALID, "need 1 <= n < 2^31 and 2 <= S <= %d (got n=%lld, S=%d)", kMaxS, (long long)n, S);
    d.n = n;
    d.S = S;
    d.gmask = 0;
    d.nA = d.nB = 0;
    for (int j = 0; j < S; j++) {
        const int g = group ? group[j] : 0;
        if (g != 0 && g != 1) return fail(c, CHICDIFF_E_INVALID, "group[%d]=%d: only two-level designs (0/1) or ~1 (all 0) are supported", j, g);
        if (g) { d.gmask |= (1ull << j); d.nB++; } else d.nA++;
    }
    d.p = d.nB > 0 ? 2 : 1;
    if (d.p == 2 && d.nA == 0) return fail(c, CHICDIFF_E_INVALID, "design has no sample in the reference level");
    if (S <= d.p) return fail(c, CHICDIFF_E_INVALID, "no residual degrees of freedom (S=%d, p=%d)", S, d.p);
    return CHICDIFF_OK;
}

// opts the caller filled in: fitType must be one of DESeq2's three (a NA_integer_ from R arrives as INT_MIN)
int cd::check_opts(chicdiff_hip_ctx *c, const chicdiff_nbglm_opts *opts) {
    if (opts && (opts->fitType < 0 || opts->fitType > 2))
        return fail(c, CHICDIFF_E_INVALID, "opts.fitType = %d: 0 (parametric), 1 (mean) or 2 (local) expected", opts->fitType);
    return CHICDIFF_OK;
}

// Sharded fits: an argument error on ONE rank (e.g. an empty shard when n < world size) must not leave its peers blocked
// in the first collective.  Every rank therefore contributes its local verdict to one sum-all-reduce before the fit
// starts, and all return together.  (Single process: the local verdict.)
static int shard_consensus(chicdiff_hip_ctx *c, int local_rc, int64_t n = 0) {
    c->shard_n_valid = false;
    if (!c->allreduce) return local_rc;
    char keep[sizeof c->err];
    memcpy(keep, c->err, sizeof keep);
    // one all-reduce carries the verdict and — zero everywhere but in the rank's own slot — the shards' row counts, which the
    // gathered trend needs (round 2 exchanged them with a collective and two host synchronisations of their own)
    const int world = c->world > 0 ? c->world : 1, slots = world <= kSelMaxWorld ? 1 + world : 1;
    double buf[1 + kSelMaxWorld] = {0};
    buf[0] = local_rc ? 1.0 : 0.0;
    if (slots > 1 && c->rank >= 0 && c->rank < world) buf[1 + c->rank] = local_rc ? 0.0 : (double)n;
    double *d_flag = c->d_sf + kMaxS;  // spare doubles behind the size factors
    hipError_t e = hipSetDevice(c->device);
    if (e == hipSuccess) e = hipMemcpyAsync(d_flag, buf, sizeof(double) * slots, hipMemcpyHostToDevice, c->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(c->stream);
    if (e != hipSuccess) return fail(c, CHICDIFF_E_HIP, "shard consensus: %s", hipGetErrorString(e));
    if (do_allreduce(c, d_flag, slots)) return CHICDIFF_E_COMM;
    e = hipMemcpyAsync(buf, d_flag, sizeof(double) * slots, hipMemcpyDeviceToHost, c->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(c->stream);
    if (e != hipSuccess) return fail(c, CHICDIFF_E_HIP, "shard consensus: %s", hipGetErrorString(e));
    const double flag = buf[0];
    if (slots > 1) {
        for (int r = 0; r < world; r++) c->shard_n[r] = buf[1 + r];
        c->shard_n_valid = flag == 0.0 && n > 0;
    }
    if (local_rc) {
        memcpy(c->err, keep, sizeof keep);
        return local_rc;
    }
    if (flag > 0) return fail(c, CHICDIFF_E_INVALID, "%d rank(s) of the sharded fit rejected their arguments (e.g. an empty shard): nothing was fitted", (int)flag);
    return CHICDIFF_OK;
}

Opts cd::make_opts(const chicdiff_hip_ctx *c, const chicdiff_nbglm_opts *in, int S) {
    chicdiff_nbglm_opts o;
    if (in) o = *in; else chicdiff_hip_default_opts(&o);
    Opts r = c->tune;
    r.minDisp = o.minDisp; r.dispTol = o.dispTol; r.kappa0 = o.kappa0; r.betaTol = o.betaTol; r.minmu = o.minmu;
    r.outlierSD = o.outlierSD; r.dispPriorVarIn = o.dispPriorVar; r.maxit = o.maxit; r.betaMaxit = o.betaMaxit;
    r.maxDisp = S > 10 ? (double)S : 10.0;
    r.trendIn[0] = o.trendCoef[0];
    r.trendIn[1] = o.trendCoef[1];
    r.fit_type = o.fitType;
    return r;
}

// ---- DESeq2 localDispersionFit on the device (trend_kernels.hip lf_*): the host grows locfit's tree ----------------
// One order statistic of key(x) or key(|x - xv|) over the rows of the fit: byte-wise radix select, eight histogram rounds
// (each a sum over rows, all-reduced when sharded).  rank is 0-based; *total gets the number of rows (first round).
static int lf_order_stat(chicdiff_hip_ctx *c, FitDims d, const Opts &o, int use_dist, double xv, double rank, double *value, double *total) {
    double *d_hist = c->w.hist;
    uint64_t prefix = 0;
    double h[256];
    for (int shift = 56; shift >= 0; shift -= 8) {
        launch_lf_hist(d, c->w, o, use_dist, xv, prefix, shift, d_hist, c->stream);
        if (int rc = do_allreduce(c, d_hist, 256)) return rc;
        HIPCHK(c, hipMemcpyAsync(h, d_hist, sizeof h, hipMemcpyDeviceToHost, c->stream));
        HIPCHK(c, hipStreamSynchronize(c->stream));
        double cum = 0;
        if (shift == 56 && total) {
            *total = 0;
            for (int b = 0; b < 256; b++) *total += h[b];
        }
        int b = 0;
        for (; b < 255; b++) {
            if (cum + h[b] > rank) break;
            cum += h[b];
        }
        rank -= cum;
        prefix |= (uint64_t)b << shift;
    }
    *value = value_of(prefix);
    return CHICDIFF_OK;
}
// bandwidth, value and slope of the local quadratic at xv (locfit: nbhd / kordstat, tricube, Taylor basis 1, dx, dx^2/2)
static int lf_vertex(chicdiff_hip_ctx *c, FitDims d, const Opts &o, double nfit, double xv, double *h, double *f, double *df) {
    const double k = floor(nfit * 0.7);  // alpha = 0.7
    if (k < 1) return CHICDIFF_E_NUMERIC;
    int rc = lf_order_stat(c, d, o, 1, xv, k - 1, h, nullptr);
    if (rc) return rc;
    if (!(*h > 0)) return CHICDIFF_E_NUMERIC;
    double *d_out = c->w.hist + 256, s[8];
    launch_lf_sums(d, c->w, o, xv, *h, c->w.partials, d_out, c->stream);
    if ((rc = do_allreduce(c, d_out, 8))) return rc;
    HIPCHK(c, hipMemcpyAsync(s, d_out, sizeof s, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    long double A[3][4] = {{s[0], s[1], (long double)s[2] / 2, s[5]},
                           {s[1], s[2], (long double)s[3] / 2, s[6]},
                           {(long double)s[2] / 2, (long double)s[3] / 2, (long double)s[4] / 4, (long double)s[7] / 2}};
    // B: the sum of the absolute values of the terms an entry was formed from.  With fewer than three distinct x inside the bandwidth
    // the exact system is singular, but the moments are rounded sums: elimination leaves a residue instead of a zero, and a test for
    // zero would take it for a pivot and fit through noise.  A pivot within kLfSingular of its terms' sum is such a residue.
    constexpr long double kLfSingular = 0x1p-40L;  // far above the moments' rounding (double sums), far below a pivot that leaves a digit
    long double B[3][4];
    for (int r = 0; r < 3; r++)
        for (int q = 0; q < 4; q++) B[r][q] = fabsl(A[r][q]);
    for (int col = 0; col < 3; col++) {
        int piv = col;
        for (int r = col + 1; r < 3; r++)
            if (fabsl(A[r][col]) > fabsl(A[piv][col])) piv = r;
        if (!(fabsl(A[piv][col]) > kLfSingular * B[piv][col])) return CHICDIFF_E_NUMERIC;
        if (piv != col)
            for (int q = 0; q < 4; q++) { std::swap(A[col][q], A[piv][q]); std::swap(B[col][q], B[piv][q]); }
        for (int r = col + 1; r < 3; r++) {
            const long double m = A[r][col] / A[col][col];
            for (int q = col; q < 4; q++) { A[r][q] -= m * A[col][q]; B[r][q] += fabsl(m) * B[col][q]; }
        }
    }
    long double b[3];
    for (int r = 2; r >= 0; r--) {
        long double t = A[r][3];
        for (int q = r + 1; q < 3; q++) t -= A[r][q] * b[q];
        b[r] = t / A[r][r];
    }
    *f = (double)b[0];
    *df = (double)b[1];
    return CHICDIFF_OK;
}
// a new vertex at xv: its index, or -1 with *rc set (CHICDIFF_E_NUMERIC: no fit possible there / too many vertices)
static int lf_add(chicdiff_hip_ctx *c, FitDims d, const Opts &o, double nfit, LfTree &t, double xv, int *rc) {
    if (t.nv >= kLfMaxV) { *rc = CHICDIFF_E_NUMERIC; return -1; }
    if ((*rc = lf_vertex(c, d, o, nfit, xv, &t.h[t.nv], &t.f[t.nv], &t.d[t.nv]))) return -1;
    t.x[t.nv] = xv;
    return t.nv++;
}
// locfit atree_grow in one dimension: cut the cell at its midpoint while its length exceeds cut = 0.8 bandwidths
static int lf_grow(chicdiff_hip_ctx *c, FitDims d, const Opts &o, double nfit, LfTree &t, int il, int ir, double range) {
    const double le = t.x[ir] - t.x[il];
    double hmin = t.h[il] > 0 ? t.h[il] : 0;
    if (t.h[ir] > 0 && (hmin == 0 || t.h[ir] < hmin)) hmin = t.h[ir];
    const double score = hmin == 0 ? 2 * le / range : le / hmin;
    if (!(0.8 < score)) return CHICDIFF_OK;
    int rc = CHICDIFF_OK;
    const int im = lf_add(c, d, o, nfit, t, (t.x[il] + t.x[ir]) / 2, &rc);
    if (im < 0) return rc;
    if ((rc = lf_grow(c, d, o, nfit, t, il, im, range))) return rc;
    return lf_grow(c, d, o, nfit, t, im, ir, range);
}
// returns CHICDIFF_OK with dispFit[] filled and the trend marked local, or CHICDIFF_E_NUMERIC when no fit is possible
// (tree_out, may be NULL: the vertices as the evaluation gets them, with their bandwidths)
static int local_trend_fit(chicdiff_hip_ctx *c, FitDims d, const Opts &o, LfTree *tree_out) {
    double lo, hi, nfit = 0, dummy;
    int rc = lf_order_stat(c, d, o, 0, 0.0, 0.0, &lo, &nfit);  // min(x) and the number of rows in the fit
    if (rc) return rc;
    if (nfit < 4) return CHICDIFF_E_NUMERIC;
    if ((rc = lf_order_stat(c, d, o, 0, 0.0, nfit - 1, &hi, &dummy))) return rc;  // max(x)
    if (!(hi > lo)) return CHICDIFF_E_NUMERIC;
    LfTree t;
    const int il = lf_add(c, d, o, nfit, t, lo, &rc), ir = il < 0 ? -1 : lf_add(c, d, o, nfit, t, hi, &rc);
    if (il < 0 || ir < 0) return rc;
    if ((rc = lf_grow(c, d, o, nfit, t, il, ir, hi - lo))) return rc;
    LfVerts v{};
    std::vector<int> order(t.nv);
    for (int i = 0; i < t.nv; i++) order[i] = i;
    std::sort(order.begin(), order.end(), [&](int p, int q) { return t.x[p] < t.x[q]; });
    v.nv = t.nv;
    for (int i = 0; i < t.nv; i++) { v.x[i] = t.x[order[i]]; v.f[i] = t.f[order[i]]; v.d[i] = t.d[order[i]]; }
    if (tree_out) {
        tree_out->nv = t.nv;
        for (int i = 0; i < t.nv; i++) { tree_out->x[i] = v.x[i]; tree_out->h[i] = t.h[order[i]]; tree_out->f[i] = v.f[i]; tree_out->d[i] = v.d[i]; }
    }
    launch_lf_eval(d, c->w, v, c->stream);
    return CHICDIFF_OK;
}

// Sharded fits: the parametric trend on ALL ranks' rows, on every rank.  The fit is ~20 dependent IRLS passes over two
// doubles per row; sharding it costs one latency-bound all-reduce per pass (20 of a sharded fit's ~38 collectives), while
// the rows themselves are small: 16 bytes each.  So the ranks exchange them once — their sizes (with the argument verdicts),
// then the rows: one all-gather of the ranks' padded (x | y) blocks (ncclAllGather, 32 MB received at 2 M rows), or, on a
// transport without an all-gather hook, a sum-all-reduce over zero-initialised all-ranks arrays (twice the bytes) — and each
// runs the single-launch persistent kernel on the whole set: one collective instead of twenty, and the trend of a sharded
// fit is bit-identical to the single-rank one (same rows, same order, same kernel).
static int gathered_trend(chicdiff_hip_ctx *c, FitDims d, const Opts &o) {
    hipStream_t st = c->stream;
    FitWork &w = c->w;
    const int real_world = c->world > 0 ? c->world : 1, rank = c->rank;
    const int fake = (real_world == 1 && c->host.bench_fake_world > 1 && c->allgather != nullptr) ? c->host.bench_fake_world : 0;  // bench hook, see HostOpts
    const int world = fake ? fake : real_world;
    std::vector<double> cnt((size_t)world, 0.0);
    int rc;
    if (fake) {
        for (int r = 0; r < world; r++) cnt[(size_t)r] = (double)d.n;
    } else if (c->shard_n_valid && world <= kSelMaxWorld && (int64_t)c->shard_n[rank] == d.n) {
        for (int r = 0; r < world; r++) cnt[(size_t)r] = c->shard_n[r];  // exchanged with the argument verdicts: no collective, no host stop
    } else {
        cnt[(size_t)rank] = (double)d.n;
        double *d_cnt = w.hist;
        HIPCHK(c, hipMemcpyAsync(d_cnt, cnt.data(), sizeof(double) * world, hipMemcpyHostToDevice, st));
        HIPCHK(c, hipStreamSynchronize(st));  // cnt lives on this frame
        if ((rc = do_allreduce(c, d_cnt, world))) return rc;
        HIPCHK(c, hipMemcpyAsync(cnt.data(), d_cnt, sizeof(double) * world, hipMemcpyDeviceToHost, st));
        HIPCHK(c, hipStreamSynchronize(st));
    }
    int64_t off = 0, total = 0, maxn = 0;
    for (int r = 0; r < world; r++) {
        if (r < rank) off += (int64_t)cnt[(size_t)r];
        total += (int64_t)cnt[(size_t)r];
        if ((int64_t)cnt[(size_t)r] > maxn) maxn = (int64_t)cnt[(size_t)r];
    }
    // layout of the gather buffer: x[total], y[total], flags[total] (int32, zero), resid[total], then — all-gather transport —
    // this rank's padded block (x[maxn] | y[maxn]) and the ranks' blocks as they arrive (world x 2 maxn)
    const bool by_gather = c->allgather != nullptr && world <= kGatherMaxWorld;
    const size_t nd = align256(sizeof(double) * (size_t)total), ni = align256(sizeof(int32_t) * (size_t)total);
    const size_t blk = align256(sizeof(double) * 2 * (size_t)maxn);
    const size_t need = 3 * nd + ni + (by_gather ? blk * (size_t)(world + 1) : 0);
    if ((rc = grow_dev(c, (void **)&c->tg_buf, &c->tg_bytes, need, 1, true, CHICDIFF_E_HIP, "hipMalloc((void **)&c->tg_buf, need)"))) return rc;
    double *xg = (double *)c->tg_buf, *yg = (double *)(c->tg_buf + nd);
    int32_t *flags = (int32_t *)(c->tg_buf + 2 * nd);
    c->tg_total = total;
    c->tg_x = xg;
    c->tg_y = yg;
    c->tg_flags = flags;
    c->tg_resid = (double *)(c->tg_buf + 2 * nd + ni);
    if (by_gather) {
        // one ncclAllGather of the ranks' (x | y) blocks, padded to the largest shard, then a copy into the contiguous all-ranks
        // arrays: half the bytes of the sum-all-reduce over zero-filled arrays it replaces, and no floating-point adds
        double *send = (double *)(c->tg_buf + 3 * nd + ni), *recv = (double *)(c->tg_buf + 3 * nd + ni + blk);
        HIPCHK(c, hipMemsetAsync(flags, 0, ni, st));
        launch_trend_gather(d, w, o, send, send + maxn, st);
        if ((rc = do_allgather(c, send, recv, (int64_t)(blk / sizeof(double))))) return rc;
        for (int r = 1; r < fake; r++)  // the other "ranks'" blocks: copies of this one's
            HIPCHK(c, hipMemcpyAsync((char *)recv + (size_t)r * blk, recv, blk, hipMemcpyDeviceToDevice, st));
        GatherLayout gl{};
        gl.world = world;
        gl.block = (int64_t)(blk / sizeof(double));
        gl.maxn = maxn;
        int64_t o2 = 0;
        for (int r = 0; r < world; r++) { gl.off[r] = o2; o2 += (int64_t)cnt[(size_t)r]; }
        gl.off[world] = o2;
        launch_trend_compact(gl, recv, xg, yg, st);
    } else {
        HIPCHK(c, hipMemsetAsync(c->tg_buf, 0, 2 * nd + ni, st));
        launch_trend_gather(d, w, o, xg + off, yg + off, st);
        if ((rc = do_allreduce(c, xg, (int64_t)(2 * nd / sizeof(double))))) return rc;  // x and y are contiguous (padding included)
    }
    FitDims dg = d;
    dg.n = total;
    FitWork wg = w;
    wg.baseMean = xg;
    wg.dispGene = yg;
    wg.allZero = flags;  // all zero: a row that does not take part carries y = NaN
    wg.resid = c->tg_resid;
    launch_trend_persistent(dg, wg, o, st, c->host.trend_mad_in_kernel != 0);
    return CHICDIFF_OK;
}

// Per-row workspace columns the caller wants back are written where the caller wants them (round 3 copied them out when the fit
// ended: two 16 MB device copies per bench step): for the duration of one fit the workspace pointers point into the caller's
// buffers; restored on every way out.
struct WorkRedirect {
    chicdiff_hip_ctx *c;
    FitWork saved;
    WorkRedirect(chicdiff_hip_ctx *c_, const chicdiff_nbglm_out *o) : c(c_), saved(c_->w) {
        if (!o) return;
        FitWork &w = c->w;
        if (o->baseMean) w.baseMean = o->baseMean;
        if (o->baseVar) w.baseVar = o->baseVar;
        if (o->dispGeneEst) w.dispGene = o->dispGeneEst;
        if (o->dispFit) w.dispFit = o->dispFit;
        if (o->dispMAP) w.dispMAP = o->dispMAP;
        if (o->dispersion) w.disp = o->dispersion;
        if (o->dispGeneIter) w.geneIter = o->dispGeneIter;
        if (o->dispIter) w.mapIter = o->dispIter;
        if (o->dispOutlier) w.outlier = o->dispOutlier;
        if (o->allZero) w.allZero = o->allZero;
    }
    ~WorkRedirect() { c->w = saved; }
};

// the prior variance is matched by simulation (prior_mc.h) instead of taken in closed form
bool cd::prior_by_simulation(const FitDims &d, const Opts &o) { return !(o.dispPriorVarIn == o.dispPriorVarIn) && d.S - d.p <= 3 && d.S > d.p; }

// residual d.f. <= 3: DESeq2 matches the prior variance by simulation (prior_mc.h).  The 200 x 40 simulated densities are
// constants (built once per process and d.f.); the matching itself runs on the device, on the histogram of the residuals in wm.resid
static int prior_mc(chicdiff_hip_ctx *c, FitDims d, FitDims dm, const FitWork &wm, bool mad_local) {
    Scope t(c, "prior_mc");
    double *d_hist = resid_hist_of(c->w);
    launch_resid_hist(dm, wm, d_hist, c->stream);
    if (!mad_local)
        if (int rc = do_allreduce(c, d_hist, kPmcBins)) return rc;
    const int df = d.S - d.p;
    if (!c->d_pmc[df]) {  // built once per process, uploaded once per context
        HIPCHK(c, hipMalloc((void **)&c->d_pmc[df], sizeof(PmcTable)));
        HIPCHK(c, hipMemcpy(c->d_pmc[df], &pmc_table(df), sizeof(PmcTable), hipMemcpyHostToDevice));
    }
    launch_prior_mc(d, c->w, d_hist, c->d_pmc[df], c->stream);
    return CHICDIFF_OK;
}

// the fit's scalars (sums and size factors included) to c->h_sc; blocks
static int read_scalars(chicdiff_hip_ctx *c) {
    HIPCHK(c, hipMemcpyAsync(c->h_sc, c->w.sc, sizeof(FitScalars), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    return CHICDIFF_OK;
}

// The global stage of a pass, between the gene-wise search and the MAP search: the trend (caller-supplied, mean, local, persistent,
// gathered or driven), the residuals, their median and MAD, and the prior variance (closed form or prior_mc).  Reads the workspace
// columns baseMean, dispGene and allZero; leaves the trend's scalars, w.resid and — under a local trend — w.dispFit.  tree (may be
// NULL): the vertices of a local trend, ascending x (nv = 0 when none was fitted).  fit_pass calls it; so does the test entry
// chicdiff_hip_selftest_global_stage_dev (selftest_api.hip), which fills the three columns from its caller's.
int cd::global_stage(chicdiff_hip_ctx *c, FitDims d, const Opts &o, bool all_rounds, LfTree *tree) {
    int rc;
    hipStream_t st = c->stream;
    FitWork &w = c->w;
    if (tree) tree->nv = 0;
    // trend: fit_driver.h runs batches of IRLS passes and polls the finished flag between batches
    bool mad_in_kernel = false;  // the persistent trend kernel went on to the residuals, their median and MAD, and the closed-form prior variance
    if (o.trendIn[0] == o.trendIn[0] && o.trendIn[1] == o.trendIn[1]) {  // caller-supplied dispersion function
        launch_trend_init(d, w, o, st);
        HIPCHK(c, hipMemcpyAsync(w.sc->coefs, o.trendIn, sizeof(double) * 2, hipMemcpyHostToDevice, st));
        HIPCHK(c, hipStreamSynchronize(st));  // o.trendIn lives on this frame
    } else if (o.fit_type == 1) {
        // fitType = "mean" (DESeq2 estimateDispersionsFit): one value for every row, the 0.1 %-trimmed mean of the gene-wise
        // estimates above 10 minDisp — an explicit, rarely used alternative, so the order statistics are taken on the host
        if (c->allreduce) return fail(c, CHICDIFF_E_INVALID, "fitType \"mean\" is not available for sharded fits");
        std::vector<double> g((size_t)d.n);
        HIPCHK(c, hipMemcpyAsync(g.data(), w.dispGene, sizeof(double) * (size_t)d.n, hipMemcpyDeviceToHost, st));
        HIPCHK(c, hipStreamSynchronize(st));
        size_t m = 0;
        for (size_t i = 0; i < g.size(); i++)
            if (g[i] > 10 * o.minDisp) g[m++] = g[i];  // NaN (all-zero rows) fails the comparison
        if (m == 0) return fail(c, CHICDIFF_E_NUMERIC, "fitType \"mean\": no gene-wise estimate above 10 * minDisp");
        // R mean(x, trim): lo = floor(n trim) + 1, hi = n + 1 - lo, mean(sort(x)[lo:hi]) with long double accumulation
        const size_t lo = (size_t)floor((double)m * 0.001), hi = m - lo;  // 0-based half-open [lo, hi)
        if (lo > 0) {
            std::nth_element(g.begin(), g.begin() + lo, g.begin() + m);
            std::nth_element(g.begin() + lo, g.begin() + (hi - 1), g.begin() + m);
        }
        long double acc = 0;
        for (size_t i = lo; i < hi; i++) acc += g[i];
        long double mean = acc / (long double)(hi - lo), t = 0;
        for (size_t i = lo; i < hi; i++) t += g[i] - mean;
        mean += t / (long double)(hi - lo);
        const double coefs[2] = {(double)mean, 0.0};
        launch_trend_init(d, w, o, st);
        HIPCHK(c, hipMemcpyAsync(w.sc->coefs, coefs, sizeof coefs, hipMemcpyHostToDevice, st));
        HIPCHK(c, hipStreamSynchronize(st));
    } else if (o.fit_type == 2) {
        // fitType = "local": on request, or — on fit_dev_impl's second pass — DESeq2's own substitute for
        // a parametric fit that failed ("a local regression fit was automatically substituted")
        Scope t(c, "trend_fit");
        launch_trend_init(d, w, o, st);
        rc = local_trend_fit(c, d, o, tree);
        if (rc == CHICDIFF_E_NUMERIC) {
            const int32_t one = 1;  // no local fit either (fewer than four usable rows): report the trend as failed
            HIPCHK(c, hipMemcpyAsync(&w.sc->failed, &one, sizeof one, hipMemcpyHostToDevice, st));
            HIPCHK(c, hipStreamSynchronize(st));
        } else if (rc)
            return rc;
    } else if (!c->allreduce && !c->no_persistent_trend && c->cu_count >= trend_persistent_blocks() && !c->host.trend_one_launch_per_pass) {
        Scope t(c, "trend_fit");  // single rank: one persistent launch (LDS-resident rows, grid barrier per IRLS pass)
        launch_trend_persistent(d, w, o, st, c->host.trend_mad_in_kernel != 0);  // no host round trip: `failed` comes back with the final scalars
        mad_in_kernel = c->host.trend_mad_in_kernel != 0;
    } else if (c->allreduce && c->host.sharded_trend_gather && !c->no_persistent_trend && c->cu_count >= trend_persistent_blocks() &&
               !c->host.trend_one_launch_per_pass) {
        Scope t(c, "trend_fit");
        if ((rc = gathered_trend(c, d, o))) return rc;
        mad_in_kernel = c->host.trend_mad_in_kernel != 0;
    } else {
        Scope t(c, "trend_fit");
        HipBackend be{c, d, o, SelArgs{}};
        const int trc = drive_trend(be);
        if (be.err) return be.err;
        if (trc == -1) return CHICDIFF_E_COMM;
        if (trc == -2) return fail(c, CHICDIFF_E_NUMERIC, "trend state machine did not finish");
    }
    if (c->host.fault_inject & 2) {  // test hook: this rank's trend kernel "lost its grid barrier"
        c->host.fault_inject &= ~2;
        launch_poke(&w.sc->failed, 3, st);
    }
    // MAD of the log residuals.  A sharded fit that gathered the trend's rows has every rank's (baseMean, dispGeneEst) on this
    // rank already: the residuals of ALL rows are formed here and the two medians (and the residual histogram of the d.f. <= 3
    // prior) are taken locally, single-rank path — no collective at all instead of eight (nine) latency-bound ones, and the
    // same bits as the one-rank fit
    const bool mad_local = c->allreduce && c->tg_total > 0;
    FitDims dm = d;
    FitWork wm = w;
    if (mad_local) {
        dm.n = c->tg_total;
        wm.baseMean = c->tg_x;
        wm.dispGene = c->tg_y;
        wm.allZero = c->tg_flags;
        wm.resid = c->tg_resid;
    }
    if (mad_in_kernel) {
        if (prior_by_simulation(d, o) && (rc = prior_mc(c, d, dm, wm, mad_local))) return rc;  // (the residuals are in wm.resid)
    } else {
        launch_dispfit_resid(dm, wm, o, st);
        SelArgs sa{};
        sa.n = dm.n;
        sa.ncol = 1;
        sa.resid = wm.resid;
        Scope t(c, "mad_select");
        sa.mode = SEL_RESID;
        if ((rc = run_select(c, sa, all_rounds, mad_local))) return rc;
        sa.mode = SEL_ABSDEV;
        if ((rc = run_select(c, sa, all_rounds, mad_local))) return rc;
        if (!prior_by_simulation(d, o)) launch_prior_var(d, w, o, st);
        else if ((rc = prior_mc(c, d, dm, wm, mad_local))) return rc;
    }
    if (c->host.fault_inject & 1) {  // test hook: this rank's select "could not fit its candidate list"
        c->host.fault_inject &= ~1;
        launch_poke(&w.sc->sel_overflow, 1, st);
    }
    return CHICDIFF_OK;
}

// one pass of a fit, from the counts to the scalars on the host (c->h_sc); fit_dev_impl reads the verdicts and repeats it if need be
static int fit_pass(chicdiff_hip_ctx *c, const int32_t *d_counts, const double *d_nf, FitDims d, const Opts &o,
                    const chicdiff_nbglm_out *d_out, bool all_rounds) {
    int rc;
    hipStream_t st = c->stream;
    FitWork &w = c->w;
    c->tg_total = 0;
    // the scalars, the queue heads and the barrier counters sit next to each other in the workspace: one fill
    HIPCHK(c, hipMemsetAsync(w.sc, 0, align256(sizeof(FitScalars)) + kQueueBytes + kBarrierBytes, st));
    // sharded: the column sums of nf travel as the ranks' double-double pairs (zero-filled slots + sum-all-reduce = an exact gather)
    // and are added in rank order — the correctly rounded exact sum, as on one rank: same xim, same start values, same bits downstream
    const int world = c->world > 0 ? c->world : 1;
    const bool col_slots = c->allreduce && world <= kSelMaxWorld;
    const size_t slot_doubles = (size_t)(d.S + 1) * 2;
    double *slots = col_slots ? w.hist : nullptr;  // (the select histograms are idle here)
    if (col_slots) HIPCHK(c, hipMemsetAsync(slots, 0, sizeof(double) * slot_doubles * world, st));
    {
        Scope t(c, "prep");
        const bool fused = c->fuse.fm != nullptr && d.S <= 16 && d_nf == c->d_nf_tmp;
        const int nblk = launch_prep(d_counts, const_cast<double *>(d_nf), d, w, o, st, fused ? c->fuse : FusedOffsets(), c->host.prep_blocks);
        launch_prep_finish(d, w, nblk, col_slots ? slots + slot_doubles * c->rank : nullptr, st);
    }
    if (col_slots) {
        if ((rc = do_allreduce(c, slots, (int64_t)(slot_doubles * world)))) return rc;
    } else if ((rc = do_allreduce(c, w.sc->colsum, kMaxS + 1)))  // colsum[kMaxS] + nnz are contiguous
        return rc;
    if (c->allreduce) launch_xim(d, w, slots, world, st);  // (the ranks' column sums, exchanged above, added in rank order -> xim)
    {
        Scope t(c, "disp_gene");
        Opts og = o;
        og.xim_here = c->allreduce ? 0 : 1;  // single rank: disp_init forms xim from the column sums itself (one dependent launch less)
        launch_disp_gene(d_counts, d_nf, d, w, og, st);
    }
    if ((rc = global_stage(c, d, o, all_rounds, nullptr))) return rc;
    {
        Scope t(c, "disp_map");
        launch_disp_map(d_counts, d_nf, d, w, o, st);
    }
    if (c->early && c->early->n > 0) {  // these columns are final: off to the host while the Wald stage runs
        const void *src[10] = {w.baseMean, w.baseVar, w.dispGene, w.dispFit, w.dispMAP, w.disp, w.geneIter, w.mapIter, w.outlier, w.allZero};
        HIPCHK(c, hipEventRecord(c->early->ready, st));
        HIPCHK(c, hipStreamWaitEvent(c->copy_stream, c->early->ready, 0));
        for (int k = 0; k < c->early->n; k++)
            HIPCHK(c, hipMemcpyAsync(c->early->item[k].pin, src[c->early->item[k].col], c->early->item[k].bytes, hipMemcpyDeviceToHost, c->copy_stream));
        HIPCHK(c, hipEventRecord(c->early->done, c->copy_stream));
        c->early->issued = true;
    }
    static const chicdiff_nbglm_out none{};
    const chicdiff_nbglm_out &out = d_out ? *d_out : none;
    if (d.p == 2) {
        {
            Scope t(c, "wald_prep");
            launch_wald_prep(d_counts, d_nf, d, w, o, st);
        }
        {
            Scope t(c, "wald_irls");
            launch_wald_irls(d_counts, d_nf, d, w, o, st);
        }
        Scope t(c, "wald_final");
        launch_wald_final(d_counts, d_nf, d, w, o, c->host.wald_final_row_constant, out, st);
    } else {
        Scope t(c, "wald_intercept");
        launch_wald_intercept(d_counts, d_nf, d, w, o, out, st);
    }
    launch_dev_sum_finish(d, w, c->d_carry, c->d_sf, st);
    // deviance sum, non-converged rows, all-zero rows, then four verdicts as rank counts: trend kernel timed out, negative / NA count,
    // a select's candidate list overflowed in this fit, ... in the size-factor select the caller ran before it
    if ((rc = do_allreduce(c, w.sc->final_sums, 7))) return rc;
    // one read brings the scalars, the sums and the size factors back (the per-row columns the caller asked for were written in place)
    if ((rc = read_scalars(c))) return rc;
    HIPCHK(c, hipGetLastError());
    return CHICDIFF_OK;
}

// estimateDispersionsFit's answer to a parametric fit that failed (read from the scalars of the pass that just ended): fitType <- "local"
bool cd::substitute_local_trend(const chicdiff_hip_ctx *c, const Opts &o) {
    return c->h_sc->failed && o.fit_type == 0 && !(o.trendIn[0] == o.trendIn[0]) && c->host.local_trend_substitute;
}

// A fit: fit_pass, repeated while the verdicts of a pass ask for it.  all_rounds: the selects take every histogram round from the
// first pass on (option "select_all_rounds", or the caller's own retry after an overflow of the size-factor select).
static int fit_dev_impl(chicdiff_hip_ctx *c, const int32_t *d_counts, const double *d_nf, FitDims d, Opts o,
                        const chicdiff_nbglm_out *d_out, chicdiff_nbglm_scalars *scalars, bool all_rounds) {
    WorkRedirect redirect(c, d_out);
    const double *hs = c->h_sc->final_sums;
    for (;;) {
        if (int rc = fit_pass(c, d_counts, d_nf, d, o, d_out, all_rounds)) return rc;
        // hs[4] is all-reduced like the other sums: a negative / NA count on ANY rank has entered everybody's size factors, trend and
        // prior, so every rank refuses the fit together (and none goes on to a retry below, whose collectives the others would miss)
        if (hs[4] > 0)
            return fail(c, CHICDIFF_E_INVALID, c->h_sc->neg_counts ? "counts contain a negative value or NA_integer_"
                                                                   : "counts contain a negative value or NA_integer_ (on another rank of the sharded fit)");
        // The verdicts below are sums over the ranks (hs[3..6]): whatever ONE rank saw, every rank takes the same branch and repeats
        // the pass together — none is left waiting in a collective its peers never issue.
        c->sf_overflow_seen = hs[6] > 0;  // the caller (wald_test_dev) repeats size factors + fit with every histogram round
        if (c->sf_overflow_seen && !all_rounds) return CHICDIFF_OK;  // (results of this pass are discarded there)
        if (hs[5] > 0 && !all_rounds) {
            all_rounds = true;  // a sharded select's candidate list did not fit: every histogram round instead
        } else if (c->h_sc->failed == 3 || hs[3] > 0) {
            // the persistent trend kernel's workgroups were not all resident within the barrier's patience (a GPU shared
            // with other work): fit again with one launch per IRLS pass, and stay with that for this context
            if (c->no_persistent_trend) return fail(c, CHICDIFF_E_HIP, "trend fit: grid barrier timed out");
            c->no_persistent_trend = true;
        } else if (substitute_local_trend(c, o)) {
            // estimateDispersionsFit: the parametric fit failed -> fitType <- "local", and the fit is done again from the trend on
            // (everything before it is recomputed too: a rare path, kept simple)
            o.fit_type = 2;
        } else
            break;
        c->refits++;
    }
    if (scalars) {
        const FitScalars *s = c->h_sc;
        int status = 0;
        if (s->failed) status |= CHICDIFF_ST_TREND_FAILED;
        if (s->trend_local) status |= CHICDIFF_ST_TREND_LOCAL;
        scalars->trendCoef[0] = s->coefs[0];
        scalars->trendCoef[1] = s->coefs[1];
        scalars->varLogDispEsts = s->varLogDispEsts;
        scalars->dispPriorVar = s->dispPriorVar;
        scalars->nAllZero = (int64_t)hs[2];
        scalars->sumDeviance = hs[2] > 0 ? NAN : hs[0];  // sum() without na.rm, chicdiff.R:1647
        scalars->trendOuterIter = s->outer_it;
        if (hs[2] > 0) status |= CHICDIFF_ST_ALLZERO_ROWS;
        if (hs[1] > 0) status |= CHICDIFF_ST_BETA_NONCONV;
        if (prior_by_simulation(d, o)) status |= CHICDIFF_ST_PRIORVAR_MC;
        scalars->status = status;
    }
    return CHICDIFF_OK;
}

// what a fit / size-factor / Wald-test call starts with: the ranks' verdicts on their arguments (rc: this rank's), the workspace
static int begin_call(chicdiff_hip_ctx *c, int rc, int64_t n, int32_t S) {
    timing_reset(c);  // (before the verdicts' collective: it is one of the call's)
    if ((rc = shard_consensus(c, rc, n))) return rc;
    HIPCHK(c, hipSetDevice(c->device));
    if ((rc = ensure_workspace(c, n, S))) return rc;
    c->refits = 0;
    return CHICDIFF_OK;
}

// The offsets of the fit that c is about to make on c->d_nf_tmp: formed from FullMean inside the fit's first kernel (c->fuse; the
// caller clears it when the fit returns), else by a launch of their own.  Inside, the nf matrix is written once and not read straight
// back (2 M x 8: 658 MB moved instead of 786), and a launch goes.  Rounds 5-17 kept that to fits of <= 2^18 rows, because at 2 M x 8
// the fused kernel took 283 us against 75 + 133 for the pair; the reasons were in the kernel, not in the idea (disp_kernels.hip,
// prep16_kernel): register arrays of 16 samples whatever S (157 registers: three workgroups per CU resident, so the 1024 of the grid
// ran as a round and a quarter), and the size factors read by 2 S vector loads per tile, each waited for on its own.  Measured since
// (round 18, one MI355X, kernel times of five steps, fused | offsets + prep of the same build): 30 k x 4 13.9 | 6.3 + 12.0 us,
// 250 k x 8 25.2 | 12.3 + 19.7, 1 M x 8 83.1 | 33.0 + 57.5, 2 M x 4 115.8 | 32.2 + 93.5, 2 M x 8 146.6 | 54.0 + 107.0,
// 2 M x 16 309.4 | 116.2 + 214.8 — ahead at every shape, outside the runs' spread, before the launch saved is counted
// (profiles/r18_routes_kernel_times.txt).
// So the rule is: inside wherever the fused kernel exists (S <= 16).  fuse_offsets = 0 keeps the pair (the bit-identity tests).
static bool fused_offsets_win(int64_t, int32_t S) { return S <= 16; }
static void form_offsets(chicdiff_hip_ctx *c, const double *d_fullMean, int64_t n, int32_t S, double theta, int mix) {
    if (d_fullMean && S <= 16 && c->host.fuse_offsets && (c->host.fuse_offsets == 2 || fused_offsets_win(n, S))) {
        c->fuse.fm = d_fullMean;
        c->fuse.sf = c->d_sf;
        c->fuse.theta = theta;
        c->fuse.mix = mix;
    } else {
        Scope t(c, "offsets");
        launch_offsets(d_fullMean, c->d_sf, n, S, theta, mix, c->d_nf_tmp, c->stream);
    }
}

extern "C" {

int chicdiff_hip_nbglm_fit_dev(chicdiff_hip_ctx *c, const int32_t *d_counts, const double *d_nf, int64_t n, int32_t S,
                               const int32_t *group, const chicdiff_nbglm_opts *opts, const chicdiff_nbglm_out *d_out,
                               chicdiff_nbglm_scalars *scalars) {
    if (!c) return CHICDIFF_E_INVALID;
    FitDims d;
    int rc = (!d_counts || !d_nf) ? fail(c, CHICDIFF_E_INVALID, "counts / nf pointer is NULL") : check_counts_group(c, n, S, group, d);
    if (!rc) rc = check_opts(c, opts);
    if ((rc = begin_call(c, rc, n, S))) return rc;
    HIPCHK(c, hipMemsetAsync(c->d_carry, 0, sizeof(int32_t), c->stream));  // no size-factor select belongs to this call
    rc = fit_dev_impl(c, d_counts, d_nf, d, make_opts(c, opts, S), d_out, scalars, c->host.select_all_rounds != 0);
    timing_collect(c);
    return rc;
}

// Host-buffer entry point (what R's .Call shim passes: INTEGER(counts), REAL(nf)).  The caller's pageable buffers go
// through a pinned staging area in slices: host threads copy a slice in (checking the counts for NA / negatives on
// the way) and enqueue its DMA at once, so the CPU copy of slice k+1 overlaps the PCIe transfer of slice k; results
// come back the same way.  Device arena and staging area live in the context and only ever grow.
int chicdiff_hip_nbglm_fit(chicdiff_hip_ctx *c, const int32_t *counts, const double *nf, int64_t n, int32_t S,
                           const int32_t *group, const chicdiff_nbglm_opts *opts, const chicdiff_nbglm_out *out,
                           chicdiff_nbglm_scalars *scalars) {
    if (!c) return CHICDIFF_E_INVALID;
    if (!counts || !nf) return fail(c, CHICDIFF_E_INVALID, "counts / nf pointer is NULL");
    if (n < 1 || S < 2 || S > kMaxS) return fail(c, CHICDIFF_E_INVALID, "need n >= 1 and 2 <= S <= %d", kMaxS);
    HIPCHK(c, hipSetDevice(c->device));
    const size_t cb = sizeof(int32_t) * (size_t)n * S, fb = sizeof(double) * (size_t)n * S;
    const size_t nd = align256(sizeof(double) * (size_t)n);
    static const chicdiff_nbglm_out none{};
    const chicdiff_nbglm_out &ho = out ? *out : none;
    double *const *hd[] = {&ho.baseMean, &ho.baseVar, &ho.dispGeneEst, &ho.dispFit, &ho.dispMAP, &ho.dispersion, &ho.log2FoldChange,
                           &ho.lfcSE, &ho.stat, &ho.pvalue, &ho.intercept, &ho.interceptSE, &ho.deviance, &ho.maxCooks};
    int32_t *const *hi[] = {&ho.dispGeneIter, &ho.dispIter, &ho.dispOutlier, &ho.betaConv, &ho.betaIter, &ho.allZero, &ho.cooksArgmax};
    int nout = 0;
    for (int k = 0; k < 14; k++) nout += *hd[k] != nullptr;
    for (int k = 0; k < 7; k++) nout += *hi[k] != nullptr;
    const size_t in_bytes = align256(cb) + align256(fb), out_bytes = nd * (size_t)nout;
    int rc = ensure_io(c, in_bytes + out_bytes, in_bytes > out_bytes ? in_bytes : out_bytes);
    if (rc) return rc;
    int32_t *d_counts = (int32_t *)c->io_dev;
    double *d_nf = (double *)(c->io_dev + align256(cb));
    char *po = c->io_dev + in_bytes;
    chicdiff_nbglm_out dout{};
    double **dd[] = {&dout.baseMean, &dout.baseVar, &dout.dispGeneEst, &dout.dispFit, &dout.dispMAP, &dout.dispersion,
                     &dout.log2FoldChange, &dout.lfcSE, &dout.stat, &dout.pvalue, &dout.intercept, &dout.interceptSE,
                     &dout.deviance, &dout.maxCooks};
    int32_t **di[] = {&dout.dispGeneIter, &dout.dispIter, &dout.dispOutlier, &dout.betaConv, &dout.betaIter, &dout.allZero, &dout.cooksArgmax};
    for (int k = 0; k < 14; k++) if (*hd[k]) { *dd[k] = (double *)po; po += nd; }
    for (int k = 0; k < 7; k++) if (*hi[k]) { *di[k] = (int32_t *)po; po += nd; }

    // ---- H2D: slices of the two input matrices, copied and enqueued by a few host threads ----
    const size_t slice = (size_t)8 << 20;
    struct Piece { const char *src; char *pin, *dev; size_t bytes; bool is_counts; };
    std::vector<Piece> pieces;
    for (size_t off = 0; off < cb; off += slice)
        pieces.push_back({(const char *)counts + off, c->io_pin + off, (char *)d_counts + off, cb - off < slice ? cb - off : slice, true});
    for (size_t off = 0; off < fb; off += slice)
        pieces.push_back({(const char *)nf + off, c->io_pin + align256(cb) + off, (char *)d_nf + off, fb - off < slice ? fb - off : slice, false});
    int nthreads = c->host.host_copy_threads;
    if ((size_t)nthreads > pieces.size()) nthreads = (int)pieces.size();
    if (nthreads < 1) nthreads = 1;
    std::vector<int64_t> bad(nthreads, -1);
    std::vector<int> trc(nthreads, 0);
    {
        std::vector<std::thread> th;
        for (int t = 0; t < nthreads; t++)
            th.emplace_back([&, t]() {
                if (hipSetDevice(c->device) != hipSuccess) { trc[t] = 1; return; }
                for (size_t k = t; k < pieces.size(); k += nthreads) {
                    const Piece &p = pieces[k];
                    if (p.is_counts) {  // copy + NA / negative check in one pass over the slice
                        const int32_t *s = (const int32_t *)p.src;
                        int32_t *d = (int32_t *)p.pin;
                        const size_t m = p.bytes / 4;
                        int32_t acc = 0;
                        for (size_t i = 0; i < m; i++) { d[i] = s[i]; acc |= s[i]; }
                        if (acc < 0 && bad[t] < 0)
                            for (size_t i = 0; i < m; i++)
                                if (s[i] < 0) { bad[t] = (int64_t)(s - counts) + (int64_t)i; break; }
                    } else
                        memcpy(p.pin, p.src, p.bytes);
                    if (hipMemcpyAsync(p.dev, p.pin, p.bytes, hipMemcpyHostToDevice, c->stream) != hipSuccess) trc[t] = 1;
                }
            });
        for (auto &w : th) w.join();
    }
    for (int t = 0; t < nthreads; t++) {
        if (bad[t] >= 0) {
            (void)hipStreamSynchronize(c->stream);
            return fail(c, CHICDIFF_E_INVALID, "counts[%lld] is negative or NA_integer_", (long long)bad[t]);
        }
        if (trc[t]) return fail(c, CHICDIFF_E_HIP, "H2D copy failed");
    }
    // ---- D2H: one DMA per column into the staging area, host threads copy out as the columns land.  The ten columns
    //      of the dispersion stage are final once the MAP estimates exist: they go over a second stream, straight from
    //      the workspace, while the Wald stage still runs (fit_dev_impl issues them); the others follow the fit ----
    struct Col { void *host; const void *dev; char *pin; size_t bytes; hipEvent_t ev; bool early; };
    std::vector<Col> cols;
    chicdiff_hip_ctx::EarlyCopy early;
    char *pp = c->io_pin;
    static const int early_of_d[14] = {0, 1, 2, 3, 4, 5, -1, -1, -1, -1, -1, -1, -1, -1}, early_of_i[7] = {6, 7, 8, -1, -1, 9, -1};
    for (int k = 0; k < 14; k++) if (*hd[k]) { cols.push_back({*hd[k], *dd[k], pp, sizeof(double) * (size_t)n, nullptr, early_of_d[k] >= 0}); if (early_of_d[k] >= 0) { early.item[early.n++] = {early_of_d[k], pp, sizeof(double) * (size_t)n}; *dd[k] = nullptr; } pp += nd; }
    for (int k = 0; k < 7; k++) if (*hi[k]) { cols.push_back({*hi[k], *di[k], pp, sizeof(int32_t) * (size_t)n, nullptr, early_of_i[k] >= 0}); if (early_of_i[k] >= 0) { early.item[early.n++] = {early_of_i[k], pp, sizeof(int32_t) * (size_t)n}; *di[k] = nullptr; } pp += nd; }
    hipError_t e = hipSuccess;
    if (early.n > 0) {
        if (!c->copy_stream) e = hipStreamCreateWithFlags(&c->copy_stream, hipStreamNonBlocking);
        if (e == hipSuccess) e = hipEventCreateWithFlags(&early.ready, hipEventDisableTiming);
        if (e == hipSuccess) e = hipEventCreateWithFlags(&early.done, hipEventDisableTiming);
        if (e != hipSuccess) return fail(c, CHICDIFF_E_HIP, "D2H setup: %s", hipGetErrorString(e));
        c->early = &early;
    }
    rc = chicdiff_hip_nbglm_fit_dev(c, d_counts, d_nf, n, S, group, opts, &dout, scalars);  // ends with a sync of the fit's stream
    c->early = nullptr;
    auto cleanup = [&]() {
        if (early.issued) (void)hipStreamSynchronize(c->copy_stream);  // the staging area must be quiet before it is reused
        if (early.ready) (void)hipEventDestroy(early.ready);
        if (early.done) (void)hipEventDestroy(early.done);
    };
    if (rc) { cleanup(); return rc; }
    for (auto &q : cols) {
        if (q.early) continue;
        if (e == hipSuccess) e = hipEventCreateWithFlags(&q.ev, hipEventDisableTiming);
        if (e == hipSuccess) e = hipMemcpyAsync(q.pin, q.dev, q.bytes, hipMemcpyDeviceToHost, c->stream);
        if (e == hipSuccess) e = hipEventRecord(q.ev, c->stream);
    }
    if (e == hipSuccess && !cols.empty()) {
        std::sort(cols.begin(), cols.end(), [](const Col &x, const Col &y) { return x.early > y.early; });  // those already on the host first
        int nt = c->host.host_copy_threads < (int)cols.size() ? c->host.host_copy_threads : (int)cols.size();
        std::vector<std::thread> th;
        for (int t = 0; t < nt; t++)
            th.emplace_back([&, t]() {
                for (size_t k = t; k < cols.size(); k += nt) {
                    if (hipEventSynchronize(cols[k].early ? early.done : cols[k].ev) != hipSuccess) { trc[0] = 1; continue; }
                    memcpy(cols[k].host, cols[k].pin, cols[k].bytes);
                }
            });
        for (auto &w : th) w.join();
    }
    for (auto &q : cols) if (q.ev) (void)hipEventDestroy(q.ev);
    cleanup();
    if (e != hipSuccess || trc[0]) return fail(c, CHICDIFF_E_HIP, "D2H copy: %s", e != hipSuccess ? hipGetErrorString(e) : "event wait failed");
    return CHICDIFF_OK;
}

// size factors -> c->d_sf (device) ; no host synchronisation.  The select's overflow verdict is left in c->d_carry (a device word
// the fit does not clear), from where the fit's last all-reduce — or sf_overflow_consensus — makes it every rank's verdict.
static int size_factors_impl(chicdiff_hip_ctx *c, const int32_t *d_counts, int64_t n, int32_t S, bool all_rounds) {
    Scope t(c, "size_factors");
    SelArgs sa{};
    sa.mode = SEL_SIZEFACTOR;
    sa.ncol = S;
    sa.n = n;
    sa.ratio = c->d_nf_tmp;
    sa.S = S;
    sa.sf_out = c->d_sf;  // the finishing step of the select writes the size factors there
    sa.overflow_out = c->d_carry;
    // (the offsets buffer is free until the size factors exist; on either route the first kernel clears the select's overflow flag,
    // c->d_carry — a device word the fit does not clear: the fit's last kernel carries it into the all-reduced verdicts)
    if (S <= kSfMaxS && !c->allreduce && !all_rounds) {
        // single rank: two passes over the counts, keys recomputed, no key matrix (global_kernels.hip).  Option "select_all_rounds"
        // = 1 — and the repeat after an overflow verdict, which only the test hook below can raise here — take the radix select.
        if (c->sfhist_dirty) HIPCHK(c, hipMemsetAsync(c->d_sfhist, 0, sizeof(unsigned int) * kSfWorkWords, c->stream));
        c->sfhist_dirty = true;
        launch_sf_direct(d_counts, n, S, sa, c->w, c->d_sfhist, reinterpret_cast<uint64_t *>(c->d_nf_tmp), c->d_carry,
                         c->cu_count, c->host.sf_log_table, c->stream);
        HIPCHK(c, hipGetLastError());
        c->sfhist_dirty = false;  // every launch went out: the pick leaves the histograms zero
    } else {
        launch_row_ratio(d_counts, n, S, c->d_nf_tmp, c->d_carry, c->stream);
        const int rc = run_select(c, sa, all_rounds);
        if (rc) return rc;
    }
    if (c->host.fault_inject & 4) {  // test hook: this rank's size-factor select "could not fit its candidate list"
        c->host.fault_inject &= ~4;
        launch_poke(c->d_carry, 1, c->stream);
    }
    return CHICDIFF_OK;
}

// did the size-factor select overflow on ANY rank?  (one 1-double sum-all-reduce when sharded; blocks)
static int sf_overflow_consensus(chicdiff_hip_ctx *c, bool *overflow) {
    double *d_flag = c->d_sf + kMaxS;  // spare doubles behind the size factors
    launch_flag_to_double(c->d_carry, d_flag, c->stream);
    int rc = do_allreduce(c, d_flag, 1);
    if (rc) return rc;
    double h = 0;
    HIPCHK(c, hipMemcpyAsync(&h, d_flag, sizeof h, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    *overflow = h > 0;
    return CHICDIFF_OK;
}

int chicdiff_hip_size_factors_dev(chicdiff_hip_ctx *c, const int32_t *d_counts, int64_t n, int32_t S, double *sf_host) {
    if (!c) return CHICDIFF_E_INVALID;
    int rc = (!d_counts || !sf_host || n < 1 || S < 1 || S > kMaxS) ? fail(c, CHICDIFF_E_INVALID, "size_factors: bad arguments") : CHICDIFF_OK;
    if ((rc = begin_call(c, rc, n, S))) return rc;
    bool all_rounds = c->host.select_all_rounds != 0, overflow = false;
    for (;;) {
        if ((rc = size_factors_impl(c, d_counts, n, S, all_rounds)) || (rc = sf_overflow_consensus(c, &overflow))) break;
        if (!overflow || all_rounds) break;
        all_rounds = true;  // a candidate list of the sharded select did not fit on some rank: every histogram round instead
        c->refits++;
    }
    if (!rc) rc = read_scalars(c);
    timing_collect(c);
    if (rc) return rc;
    for (int j = 0; j < S; j++) {
        if (c->h_sc->sel_count[j] <= 0)
            return fail(c, CHICDIFF_E_NUMERIC, "every gene contains at least one zero, cannot compute log geometric means");
        sf_host[j] = c->h_sc->sel_value[2 * j];
    }
    return CHICDIFF_OK;
}

// a5 + a4 + a6 + a7 in one enqueue: estimateSizeFactors -> sc(theta) -> estimateDispersions -> nbinomWaldTest
// (chicdiff.R:1561-1562, 1666-1674) with the size factors and offsets never leaving HBM.
int chicdiff_hip_wald_test_dev(chicdiff_hip_ctx *c, const int32_t *d_counts, const double *d_fullMean, int64_t n, int32_t S,
                               const int32_t *group, double theta, const chicdiff_nbglm_opts *opts,
                               const chicdiff_nbglm_out *d_out, chicdiff_nbglm_scalars *scalars, double *sf_host) {
    if (!c) return CHICDIFF_E_INVALID;
    FitDims d;
    int rc = !d_counts ? fail(c, CHICDIFF_E_INVALID, "counts pointer is NULL") : check_counts_group(c, n, S, group, d);
    if (!rc) rc = check_opts(c, opts);
    if ((rc = begin_call(c, rc, n, S))) return rc;
    const Opts o = make_opts(c, opts, S);
    const int mix = theta == theta;
    bool all_rounds = c->host.select_all_rounds != 0;
    for (;;) {
        if ((rc = size_factors_impl(c, d_counts, n, S, all_rounds))) break;
        form_offsets(c, d_fullMean, n, S, mix ? theta : 0.0, mix);
        rc = fit_dev_impl(c, d_counts, c->d_nf_tmp, d, o, d_out, scalars, all_rounds);  // ends with a stream sync; the size factors come back with its scalars
        c->fuse = FusedOffsets();
        // the sharded size-factor select ran without a host look at its candidate lists: one that did not fit on ANY rank (massive
        // ties) shows in the fit's last all-reduce, on every rank alike, and the call is repeated with every histogram round
        if (rc || !c->sf_overflow_seen || all_rounds) break;
        all_rounds = true;
        c->refits++;
    }
    timing_collect(c);
    if (rc) return rc;
    for (int j = 0; j < S; j++) {
        if (!(c->h_sc->final_sf[j] == c->h_sc->final_sf[j]))
            return fail(c, CHICDIFF_E_NUMERIC, "every gene contains at least one zero, cannot compute log geometric means");
        if (sf_host) sf_host[j] = c->h_sc->final_sf[j];
    }
    return CHICDIFF_OK;
}

int chicdiff_hip_offsets_dev(chicdiff_hip_ctx *c, const double *d_fullMean, const double *sf_host, int64_t n, int32_t S,
                             double theta, double *d_nf_out) {
    if (!c) return CHICDIFF_E_INVALID;
    if (!sf_host || !d_nf_out || n < 1 || S < 1 || S > kMaxS) return fail(c, CHICDIFF_E_INVALID, "offsets: bad arguments");
    HIPCHK(c, hipSetDevice(c->device));
    timing_reset(c);
    HIPCHK(c, hipMemcpyAsync(c->d_sf, sf_host, sizeof(double) * S, hipMemcpyHostToDevice, c->stream));
    const int mix = theta == theta;
    {
        Scope t(c, "offsets");
        launch_offsets(d_fullMean, c->d_sf, n, S, mix ? theta : 0.0, mix, d_nf_out, c->stream);
    }
    HIPCHK(c, hipStreamSynchronize(c->stream));  // sf_host may be a temporary
    timing_collect(c);
    return CHICDIFF_OK;
}

int chicdiff_hip_theta_grid_dev(chicdiff_hip_ctx *c, const int32_t *d_counts, const double *d_fullMean, const double *sf_host,
                                int64_t n, int32_t S, const double *thetas, int32_t ntheta, const chicdiff_nbglm_opts *opts,
                                double *deviances_host) {
    if (!c) return CHICDIFF_E_INVALID;
    FitDims d;
    int rc = (!d_counts || !d_fullMean || !sf_host || !thetas || !deviances_host || ntheta < 1)
                 ? fail(c, CHICDIFF_E_INVALID, "theta_grid: bad arguments")
                 : check_counts_group(c, n, S, nullptr, d);  // design ~ 1  ("sic!", chicdiff.R:1629-1631)
    if (!rc) rc = check_opts(c, opts);
    if ((rc = shard_consensus(c, rc, n))) return rc;
    HIPCHK(c, hipSetDevice(c->device));
    timing_reset(c);
    const Opts o = make_opts(c, opts, S);  // (the parent's: the concurrent fits below run with it too)
    const bool all_rounds = c->host.select_all_rounds != 0;
    // Single rank: the |Grid| fits are independent, so they run on child contexts (own stream + workspace), up to
    // theta_grid_concurrency at once, each driven by its own host thread: one fit's straggler tail and its latency-bound
    // global steps (trend barriers, selects) overlap with the other fits' line searches.  Sharded: one after the other
    // (every rank must issue its collectives in the same order).
    const size_t ws_per_lane = sizeof(double) * (size_t)n * (26 + S) + (size_t)row_stride(S) * (size_t)n + (64u << 20);
    int lanes = c->allreduce ? 1 : (ntheta < c->host.theta_grid_concurrency ? ntheta : c->host.theta_grid_concurrency);
    bool squeezed = false;  // the lanes' workspaces do not fit: their memory is given back before the thetas are fitted one after the other
    if (lanes > 1) {
        // the lanes' workspaces must fit what the device has free NOW (a shared GPU, the caller's own tensors, a smaller
        // part); lanes that already hold a workspace of this size cost nothing more
        size_t free_b = 0, total_b = 0;
        HIPCHK(c, hipMemGetInfo(&free_b, &total_b));
        int have = 0;
        for (chicdiff_hip_ctx *l : c->lanes) have += (l->cap_n >= n && l->cap_S >= S) ? 1 : 0;
        while (lanes > 1 && lanes > have && (double)ws_per_lane * (lanes - have) > 0.9 * (double)free_b) {
            lanes--;
            squeezed = lanes <= 1;
        }
    }
    while (lanes > 1 && (int)c->lanes.size() < lanes) {
        chicdiff_hip_ctx *l = nullptr;
        if (chicdiff_hip_create(&l, c->device)) { lanes = 1; squeezed = true; break; }
        c->lanes.push_back(l);
    }
    for (int k = 0; k < lanes && lanes > 1; k++)
        if (ensure_workspace(c->lanes[k], n, S)) {  // no room after all
            snprintf(c->err, sizeof c->err, "theta_grid: concurrent fits given up (%s)", c->lanes[k]->err);  // kept for the caller's log; the call goes on
            lanes = 1;
            squeezed = true;
        }
    if (lanes <= 1) {
        // (a caller who simply asked for one lane — ntheta == 1, theta_grid_concurrency 1 — keeps the cached lanes: re-creating
        // them costs streams, GBs of hipMalloc and event-pool warm-up on the next multi-theta call)
        if (squeezed && !c->lanes.empty()) {
            for (chicdiff_hip_ctx *l : c->lanes) chicdiff_hip_destroy(l);
            c->lanes.clear();
        }
        rc = ensure_workspace(c, n, S);
        if (rc == CHICDIFF_E_NOMEM && !c->lanes.empty()) {  // the cached lanes hold whole workspaces of their own: give them up and try once more
            for (chicdiff_hip_ctx *l : c->lanes) chicdiff_hip_destroy(l);
            c->lanes.clear();
            rc = ensure_workspace(c, n, S);
        }
        if (rc) return rc;
        HIPCHK(c, hipMemsetAsync(c->d_carry, 0, sizeof(int32_t), c->stream));  // no size-factor select belongs to this call
        HIPCHK(c, hipMemcpyAsync(c->d_sf, sf_host, sizeof(double) * S, hipMemcpyHostToDevice, c->stream));
        for (int t = 0; t < ntheta; t++) {
            form_offsets(c, d_fullMean, n, S, thetas[t], 1);
            chicdiff_nbglm_scalars sc;
            rc = fit_dev_impl(c, d_counts, c->d_nf_tmp, d, o, nullptr, &sc, all_rounds);
            c->fuse = FusedOffsets();
            if (rc) return rc;
            deviances_host[t] = sc.sumDeviance;
        }
        timing_collect(c);
        return CHICDIFF_OK;
    }
    hipEvent_t ready;  // the inputs are produced on the caller's stream
    HIPCHK(c, hipEventCreateWithFlags(&ready, hipEventDisableTiming));
    HIPCHK(c, hipEventRecord(ready, c->stream));
    std::vector<int> lane_rc(lanes, CHICDIFF_OK);
    std::vector<std::thread> workers;
    for (int k = 0; k < lanes; k++) {
        chicdiff_hip_ctx *l = c->lanes[k];
        l->host = c->host;  // the host-side options; the kernels' (Opts) are the parent's: `o` above
        l->host.fault_inject = 0;  // (the one-shot bits are the parent's, for a call of its own)
        // a grid barrier needs its workgroups co-resident: not guaranteed beside other fits.  (Measured, round 4: the lanes' trend as
        // the single-launch kernel capped at 16 / 32 / 64 workgroups — 2 M x 8, five thetas: 2 lanes 16.5 -> 18.2 ms, 3 lanes 17.2 ->
        // 17.9, 5 lanes 16.3 ms -> 5-13 SECONDS: the kernel's workgroups wait for LDS that the other lanes' line-search workgroups
        // hold until their launch ends, and the barrier spins meanwhile.  With the uncapped kernel and a host mutex so that only one
        // lane's trend kernel is in flight at a time: 5 lanes 16.2 -> 18.1 ms.  A kernel trace of the grid (tools/theta_grid_trace.py)
        // shows why nothing small overlaps: while a line-search launch is resident, the other streams' small kernels do not start at
        // all — they run in the gaps between the big launches.  One launch per IRLS pass it stays.)
        l->no_persistent_trend = true;
        workers.emplace_back([=, &lane_rc]() {
            int r = CHICDIFF_OK;
            if (hipSetDevice(l->device) != hipSuccess || hipStreamWaitEvent(l->stream, ready, 0) != hipSuccess) r = CHICDIFF_E_HIP;
            if (!r) r = ensure_workspace(l, n, S);
            if (!r && hipMemcpyAsync(l->d_sf, sf_host, sizeof(double) * S, hipMemcpyHostToDevice, l->stream) != hipSuccess) r = CHICDIFF_E_HIP;
            for (int t = k; t < ntheta && !r; t += lanes) {
                form_offsets(l, d_fullMean, n, S, thetas[t], 1);
                chicdiff_nbglm_scalars sc;
                r = fit_dev_impl(l, d_counts, l->d_nf_tmp, d, o, nullptr, &sc, all_rounds);
                l->fuse = FusedOffsets();
                if (!r) deviances_host[t] = sc.sumDeviance;
            }
            lane_rc[k] = r;
        });
    }
    for (auto &w : workers) w.join();
    (void)hipEventDestroy(ready);
    for (int k = 0; k < lanes; k++)
        if (lane_rc[k]) return fail(c, lane_rc[k], "theta_grid: %s", c->lanes[k]->err[0] ? c->lanes[k]->err : "a concurrent fit failed");
    timing_collect(c);
    return CHICDIFF_OK;
}

}  // extern "C"
