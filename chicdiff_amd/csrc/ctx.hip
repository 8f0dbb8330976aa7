// ctx.hip — the context of include/chicdiff_hip.h: options, streams, the collective transports, timers, the workspace and the other
// grow-only buffers, device memory for hosts without GPU arrays of their own.  What the other host sources share is declared in ctx.h.
#include <stdarg.h>

#include <dlfcn.h>

#include "ctx.h"

char cd::g_create_err[512];

// simulated residual densities + loess operator of one d.f. (prior_mc.h): constants, built once per process
const PmcTable &cd::pmc_table(int df) {
    static PmcTable tables[4];
    static bool ready[4] = {false, false, false, false};
    static std::mutex mu;
    std::lock_guard<std::mutex> lock(mu);
    if (!ready[df]) {
        pmc_build(df, tables[df]);
        ready[df] = true;
    }
    return tables[df];
}

int cd::fail(chicdiff_hip_ctx *c, int code, const char *fmt, ...) {
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(c ? c->err : g_create_err, 512, fmt, ap);
    va_end(ap);
    return code;
}

extern "C" {

const char *chicdiff_hip_last_error(const chicdiff_hip_ctx *ctx) { return ctx ? ctx->err : g_create_err; }

void chicdiff_hip_default_opts(chicdiff_nbglm_opts *o) {
    o->minDisp = 1e-8;
    o->dispTol = 1e-6;
    o->kappa0 = 1.0;
    o->maxit = 100;
    o->betaMaxit = 100;
    o->betaTol = 1e-8;
    o->minmu = 0.5;
    o->outlierSD = 2.0;
    o->dispPriorVar = NAN;
    o->trendCoef[0] = o->trendCoef[1] = NAN;
    o->fitType = 0;
    o->_pad = 0;
}

// Every option of chicdiff_hip_set_option, in the order of the list in include/chicdiff_hip.h (tests/test_cabi.py compares the
// two): where its value is stored (a field of ctx->tune or of ctx->host), the range it accepts, and the values inside that
// range it refuses (no_lo .. no_hi; none where no_lo > no_hi).  Retiring an option is deleting its line here and there.
struct OptionDef {
    const char *name;
    int32_t Opts::*tune;
    int HostOpts::*host;
    int64_t lo, hi, no_lo, no_hi;
};
static const OptionDef kOptions[] = {
    {"line_search_spread", &Opts::spread, nullptr, 0, 3, 1, 0},  // 2: samples across lanes without the lean tick of the launch's end (bit-identity tests)
    {"line_search_min_waves", &Opts::min_waves, nullptr, 0, 4, 1, 1},  // 0 (by rule) or 2 .. 4
    {"line_search_chunk", &Opts::chunk, nullptr, 0, 64, 1, 7},         // 0 (automatic) or 8 .. 64
    {"line_search_prio", &Opts::prio, nullptr, 0, 100, 1, 0},
    {"line_search_schedule", &Opts::schedule, nullptr, 0, 4, 2, 2},    // 0, 1, kSchedSix, kSchedMinDispLast; 2 is not a mode
    {"line_search_deal", &Opts::deal, nullptr, 0, 64, 1, 0},
    {"line_search_classes_a", &Opts::classes_a, nullptr, 0, 6, 1, 0},
    {"line_search_fillers", &Opts::fillers, nullptr, -1, 1, 1, 0},
    {"line_search_filler_stop", &Opts::filler_stop, nullptr, -1, 100, 1, 0},
    {"theta_grid_concurrency", nullptr, &HostOpts::theta_grid_concurrency, 1, 16, 1, 0},
    {"host_copy_threads", nullptr, &HostOpts::host_copy_threads, 1, 64, 1, 0},
    {"select_all_rounds", nullptr, &HostOpts::select_all_rounds, 0, 1, 1, 0},
    {"trend_one_launch_per_pass", nullptr, &HostOpts::trend_one_launch_per_pass, 0, 1, 1, 0},
    {"sharded_trend_gather", nullptr, &HostOpts::sharded_trend_gather, 0, 1, 1, 0},
    {"trend_persistent_blocks", &Opts::trend_blocks, nullptr, 0, 256, 1, 0},
    {"trend_speculate", &Opts::trend_speculate, nullptr, 0, 1, 1, 0},
    {"trend_exchange", &Opts::trend_exchange, nullptr, 0, 1, 1, 0},
    {"mad_select_route", &Opts::mad_route, nullptr, 0, 1, 1, 0},
    {"mad_value_cap", &Opts::mad_value_cap, nullptr, 0, kVbCap, 1, 0},
    {"trend_mad_in_kernel", nullptr, &HostOpts::trend_mad_in_kernel, 0, 1, 1, 0},
    {"fuse_offsets", nullptr, &HostOpts::fuse_offsets, 0, 2, 1, 0},
    {"prep_blocks", nullptr, &HostOpts::prep_blocks, 0, kRedBlocks, 1, 0},
    {"region_assemble_generic", nullptr, &HostOpts::region_assemble_generic, 0, 1, 1, 0},
    {"chicago_tables_run_merge", nullptr, &HostOpts::chicago_tables_run_merge, 0, 1, 1, 0},
    {"table_write_half_kib", nullptr, &HostOpts::table_write_half_kib, 0, 65536, 1, 3},  // 0 (64 MiB at most) or 4 .. 65536
    {"fault_inject", nullptr, &HostOpts::fault_inject, 0, 7, 1, 0},
    {"bench_fake_world", nullptr, &HostOpts::bench_fake_world, 0, kGatherMaxWorld, 1, 0},
    {"sf_log_table", nullptr, &HostOpts::sf_log_table, 0, 1, 1, 0},
    {"wald_final_row_constant", nullptr, &HostOpts::wald_final_row_constant, 0, 1, 1, 0},
    {"local_trend_substitute", nullptr, &HostOpts::local_trend_substitute, 0, 1, 1, 0},
};

int chicdiff_hip_set_option(chicdiff_hip_ctx *c, const char *name, int64_t value) {
    if (!c || !name) return CHICDIFF_E_INVALID;
    for (const OptionDef &d : kOptions) {
        if (strcmp(name, d.name) != 0 || value < d.lo || value > d.hi || (value >= d.no_lo && value <= d.no_hi)) continue;
        // a rehearsal hook of bench.py, not an option of the product: refused unless the process says it is that rehearsal
        // (it makes a 1-rank fit's trend run on N copies of its rows — a fit nobody asked for)
        if (d.host == &HostOpts::bench_fake_world && value > 1 && !getenv("CHICDIFF_BENCH_FAKE_WORLD"))
            return fail(c, CHICDIFF_E_INVALID, "set_option: bench_fake_world is a rehearsal hook of bench.py (CHICDIFF_BENCH_FAKE_WORLD unset)");
        if (d.tune) c->tune.*d.tune = (int32_t)value;
        else c->host.*d.host = (int)value;
        return CHICDIFF_OK;
    }
    return fail(c, CHICDIFF_E_INVALID, "set_option: unknown option or value (%s = %lld)", name, (long long)value);
}

int chicdiff_hip_create(chicdiff_hip_ctx **out, int32_t device) {
    if (!out) return fail(nullptr, CHICDIFF_E_INVALID, "ctx out pointer is NULL");
    *out = nullptr;
    int ndev = 0;
    hipError_t e = hipGetDeviceCount(&ndev);
    if (e != hipSuccess || ndev <= 0)
        return fail(nullptr, CHICDIFF_E_HIP, "no HIP device available (%s): the HIP path cannot run, and there is no CPU fallback",
                    e != hipSuccess ? hipGetErrorString(e) : "device count 0");
    if (device < 0 || device >= ndev) return fail(nullptr, CHICDIFF_E_INVALID, "device %d out of range [0,%d)", device, ndev);
    chicdiff_hip_ctx *c = new chicdiff_hip_ctx();
    c->device = device;
    if ((e = hipSetDevice(device)) != hipSuccess || (e = hipStreamCreateWithFlags(&c->own_stream, hipStreamNonBlocking)) != hipSuccess ||
        (e = hipHostMalloc((void **)&c->h_sc, sizeof(FitScalars))) != hipSuccess ||
        (e = hipHostMalloc((void **)&c->h_sf, sizeof(double) * (kMaxS + 1))) != hipSuccess ||
        (e = hipMalloc((void **)&c->d_sf, sizeof(double) * (kMaxS + 1 + kSelMaxWorld + 8))) != hipSuccess ||
        (e = hipMemset(c->d_sf, 0, sizeof(double) * (kMaxS + 1 + kSelMaxWorld + 8))) != hipSuccess ||
        (e = hipMalloc((void **)&c->d_logfact, sizeof(double) * kLogFactN)) != hipSuccess) {
        fail(nullptr, CHICDIFF_E_HIP, "context setup: %s", hipGetErrorString(e));
        delete c;
        return CHICDIFF_E_HIP;
    }
    {
        hipDeviceProp_t prop;
        if (hipGetDeviceProperties(&prop, device) == hipSuccess) c->cu_count = prop.multiProcessorCount;
    }
    {  // log(k!) for k < kLogFactN: lgamma(y + 1) of the NB log-likelihood's constant part is a table look-up for ordinary counts
        std::vector<double> lf(kLogFactN);
        for (int k = 0; k < kLogFactN; k++) lf[k] = lgamma((double)k + 1.0);
        if ((e = hipMemcpy(c->d_logfact, lf.data(), sizeof(double) * kLogFactN, hipMemcpyHostToDevice)) != hipSuccess) {
            fail(nullptr, CHICDIFF_E_HIP, "context setup: %s", hipGetErrorString(e));
            chicdiff_hip_destroy(c);
            return CHICDIFF_E_HIP;
        }
    }
    c->d_carry = reinterpret_cast<int32_t *>(c->d_sf + kMaxS + 1 + kSelMaxWorld);  // (zeroed above)
    c->stream = c->own_stream;
    *out = c;
    return CHICDIFF_OK;
}

void chicdiff_hip_destroy(chicdiff_hip_ctx *c) {
    if (!c) return;
    (void)hipSetDevice(c->device);
    (void)hipStreamSynchronize(c->stream);
    for (auto e : c->event_pool) (void)hipEventDestroy(e);
    delete c->chin;
    if (c->chin_text) (void)hipFree(c->chin_text);
    if (c->chin_cols) (void)hipFree(c->chin_cols);
    if (c->pk_buf) (void)hipFree(c->pk_buf);
    if (c->tt_text) (void)hipFree(c->tt_text);
    if (c->chin_pin) (void)hipHostFree(c->chin_pin);
    for (hipEvent_t e : c->chin_ev)
        if (e) (void)hipEventDestroy(e);
    for (void *p : c->user_allocs) (void)hipFree(p);
    c->user_allocs.clear();
    if (c->io_dev) (void)hipFree(c->io_dev);
    if (c->io_pin) (void)hipHostFree(c->io_pin);
    for (auto *l : c->lanes) chicdiff_hip_destroy(l);
    c->lanes.clear();
    if (c->ws) (void)hipFree(c->ws);
    if (c->aux) (void)hipFree(c->aux);
    if (c->tg_buf) (void)hipFree(c->tg_buf);
    if (c->d_sf) (void)hipFree(c->d_sf);
    if (c->d_logfact) (void)hipFree(c->d_logfact);
    for (int k = 0; k < 4; k++)
        if (c->d_pmc[k]) (void)hipFree(c->d_pmc[k]);
    if (c->h_sc) (void)hipHostFree(c->h_sc);
    if (c->h_sf) (void)hipHostFree(c->h_sf);
    if (c->rccl_comm && c->rccl_comm_destroy) (void)c->rccl_comm_destroy(c->rccl_comm);
    if (c->ev_fork) (void)hipEventDestroy(c->ev_fork);
    if (c->ev_join) (void)hipEventDestroy(c->ev_join);
    if (c->copy_stream) (void)hipStreamDestroy(c->copy_stream);
    if (c->own_stream) (void)hipStreamDestroy(c->own_stream);
    delete c;
}

int chicdiff_hip_set_stream(chicdiff_hip_ctx *c, void *s) {
    if (!c) return CHICDIFF_E_INVALID;
    c->stream = (hipStream_t)s;  // NULL is HIP's null stream (what torch calls the default stream)
    return CHICDIFF_OK;
}

int chicdiff_hip_set_allreduce(chicdiff_hip_ctx *c, chicdiff_allreduce_fn fn, void *user, int32_t world, int32_t rank) {
    if (!c || world < 1 || rank < 0 || rank >= world || (world > 1 && !fn))
        return fail(c, CHICDIFF_E_INVALID, "set_allreduce: bad arguments");
    c->allreduce = fn;
    c->allreduce_user = user;
    c->allgather = nullptr;  // belongs to the transport that was replaced; set it again with chicdiff_hip_set_allgather
    c->allgather_user = nullptr;
    c->world = world;
    c->rank = rank;
    return CHICDIFF_OK;
}

int chicdiff_hip_set_allgather(chicdiff_hip_ctx *c, chicdiff_allgather_fn fn, void *user) {
    if (!c) return CHICDIFF_E_INVALID;
    if (fn && !c->allreduce) return fail(c, CHICDIFF_E_INVALID, "set_allgather: register the all-reduce of the same transport first");
    c->allgather = fn;
    c->allgather_user = user;
    return CHICDIFF_OK;
}

int32_t chicdiff_hip_last_refits(const chicdiff_hip_ctx *c) { return c ? c->refits : 0; }

// ---- direct RCCL: the library calls ncclAllReduce itself on its own stream (no host callback per collective) ----
struct RcclUniqueId { char internal[128]; };  // NCCL_UNIQUE_ID_BYTES
static int rccl_open(chicdiff_hip_ctx *c, const char *path) {
    if (c->rccl_lib) return CHICDIFF_OK;
    void *h = dlopen(path && path[0] ? path : "librccl.so", RTLD_NOW | RTLD_LOCAL);
    if (!h) return fail(c, CHICDIFF_E_COMM, "dlopen(%s): %s", path && path[0] ? path : "librccl.so", dlerror());
    c->rccl_lib = h;
    return CHICDIFF_OK;
}
// what the library's own RCCL callbacks return after a failure: the message is in c->err already (a host callback returns any other
// non-zero value and gets the generic text — round 4 told the two apart by looking for "nccl" in c->err, which a stale message
// from an earlier call satisfied just as well: ADVICE r04)
constexpr int kCollMsgSet = 0x7e57;
static int rccl_allreduce_cb(void *user, void *dev_buf, int64_t count) {
    chicdiff_hip_ctx *c = (chicdiff_hip_ctx *)user;
    const int r = c->rccl_allreduce(dev_buf, dev_buf, (size_t)count, /*ncclFloat64*/ 8, /*ncclSum*/ 0, c->rccl_comm, c->stream);
    if (r != 0) {
        fail(c, CHICDIFF_E_COMM, "ncclAllReduce: %s", c->rccl_error_string ? c->rccl_error_string(r) : "error");
        return kCollMsgSet;
    }
    return 0;
}
static int rccl_allgather_cb(void *user, const void *dev_send, void *dev_recv, int64_t count) {
    chicdiff_hip_ctx *c = (chicdiff_hip_ctx *)user;
    const int r = c->rccl_allgather(dev_send, dev_recv, (size_t)count, /*ncclFloat64*/ 8, c->rccl_comm, c->stream);
    if (r != 0) {
        fail(c, CHICDIFF_E_COMM, "ncclAllGather: %s", c->rccl_error_string ? c->rccl_error_string(r) : "error");
        return kCollMsgSet;
    }
    return 0;
}
int chicdiff_hip_rccl_unique_id(chicdiff_hip_ctx *c, const char *librccl_path, void *id128) {
    if (!c || !id128) return CHICDIFF_E_INVALID;
    int rc = rccl_open(c, librccl_path);
    if (rc) return rc;
    auto get = (int (*)(RcclUniqueId *))dlsym(c->rccl_lib, "ncclGetUniqueId");
    if (!get) return fail(c, CHICDIFF_E_COMM, "librccl lacks ncclGetUniqueId");
    const int r = get((RcclUniqueId *)id128);
    if (r != 0) return fail(c, CHICDIFF_E_COMM, "ncclGetUniqueId failed (%d)", r);
    return CHICDIFF_OK;
}
int chicdiff_hip_rccl_init(chicdiff_hip_ctx *c, const char *librccl_path, const void *id128, int32_t world, int32_t rank) {
    if (!c || !id128 || world < 1 || rank < 0 || rank >= world) return fail(c, CHICDIFF_E_INVALID, "rccl_init: bad arguments");
    int rc = rccl_open(c, librccl_path);
    if (rc) return rc;
    HIPCHK(c, hipSetDevice(c->device));
    auto init = (int (*)(void **, int, RcclUniqueId, int))dlsym(c->rccl_lib, "ncclCommInitRank");
    c->rccl_allreduce = (int (*)(const void *, void *, size_t, int, int, void *, hipStream_t))dlsym(c->rccl_lib, "ncclAllReduce");
    c->rccl_allgather = (int (*)(const void *, void *, size_t, int, void *, hipStream_t))dlsym(c->rccl_lib, "ncclAllGather");
    c->rccl_comm_destroy = (int (*)(void *))dlsym(c->rccl_lib, "ncclCommDestroy");
    c->rccl_error_string = (const char *(*)(int))dlsym(c->rccl_lib, "ncclGetErrorString");
    if (!init || !c->rccl_allreduce || !c->rccl_comm_destroy) return fail(c, CHICDIFF_E_COMM, "librccl lacks ncclCommInitRank / ncclAllReduce / ncclCommDestroy");
    if (c->rccl_comm) {
        (void)c->rccl_comm_destroy(c->rccl_comm);
        c->rccl_comm = nullptr;
    }
    RcclUniqueId id;
    memcpy(&id, id128, sizeof id);
    const int r = init(&c->rccl_comm, world, id, rank);
    if (r != 0) {
        c->rccl_comm = nullptr;
        return fail(c, CHICDIFF_E_COMM, "ncclCommInitRank: %s", c->rccl_error_string ? c->rccl_error_string(r) : "error");
    }
    c->allreduce = rccl_allreduce_cb;
    c->allreduce_user = c;
    c->allgather = c->rccl_allgather ? rccl_allgather_cb : nullptr;  // (a librccl without it: the sum-all-reduce way of gathering)
    c->allgather_user = c;
    c->world = world;
    c->rank = rank;
    return CHICDIFF_OK;
}

int chicdiff_hip_enable_timing(chicdiff_hip_ctx *c, int32_t on) {
    if (!c) return CHICDIFF_E_INVALID;
    c->timing = (on == 2 || on == 3) ? on : (on != 0 ? 1 : 0);
    return CHICDIFF_OK;
}

}  // extern "C"

// ---- timing (Scope: ctx.h) ----------------------------------------------------------------
int cd::timer_slot(chicdiff_hip_ctx *c, const char *name) {
    for (size_t i = 0; i < c->timers.size(); i++)
        if (c->timers[i].name == name) return (int)i;
    KTimer t;
    t.name = name;
    c->timers.push_back(t);
    return (int)c->timers.size() - 1;
}
hipEvent_t cd::take_event(chicdiff_hip_ctx *c) {
    hipEvent_t e = nullptr;
    if (!c->event_pool.empty()) {
        e = c->event_pool.back();
        c->event_pool.pop_back();
    } else {
        (void)hipEventCreate(&e);
    }
    return e;
}
void cd::timing_reset(chicdiff_hip_ctx *c) {
    for (auto &t : c->timers) {
        t.ms = 0;
        t.launches = 0;
        t.bytes = 0;
    }
}
void cd::timing_collect(chicdiff_hip_ctx *c) {
    if (!c->timing) return;
    (void)hipStreamSynchronize(c->stream);
    for (size_t i = 0; i + 1 < c->pending.size(); i += 2) {
        float ms = 0;
        (void)hipEventElapsedTime(&ms, c->pending[i].second, c->pending[i + 1].second);
        c->timers[c->pending[i].first].ms += ms;
        c->timers[c->pending[i].first].launches++;
        c->event_pool.push_back(c->pending[i].second);
        c->event_pool.push_back(c->pending[i + 1].second);
    }
    c->pending.clear();
}

extern "C" int32_t chicdiff_hip_kernel_times(chicdiff_hip_ctx *c, chicdiff_kernel_time *out, int32_t cap) {
    if (!c) return 0;
    int32_t k = 0;
    for (auto &t : c->timers) {
        if (t.launches == 0) continue;
        if (out && k < cap) {
            out[k].name = t.name.c_str();
            out[k].ms = t.ms;
            out[k].launches = t.launches;
            out[k].bytes = t.bytes;
        }
        k++;
    }
    return k;
}

// ---- workspace --------------------------------------------------------------------------
int cd::ensure_workspace(chicdiff_hip_ctx *c, int64_t n, int S) {
    if (c->ws && n <= c->cap_n && S <= c->cap_S) return CHICDIFF_OK;
    if (c->ws) {
        HIPCHK(c, hipStreamSynchronize(c->stream));
        HIPCHK(c, hipFree(c->ws));
        c->ws = nullptr;
    }
    const size_t nd = align256(sizeof(double) * (size_t)n), ni = align256(sizeof(int32_t) * (size_t)n);
    const size_t n_double_arrays = 15, n_int_arrays = 9;
    const size_t partials = align256(sizeof(double) * ((size_t)kRedBlocks * 72 + 128));  // the block partials, then the sums (common.h sums_of)
    const size_t hist = align256(sizeof(double) * (size_t)kMaxS * 2 * kSelBins);
    const size_t nfbytes = align256(sizeof(double) * (size_t)n * S);
    const size_t selcnt = align256(sizeof(double) * (size_t)kSelMaxWorld * kMaxS * 2);
    const size_t rowpack = align256((size_t)row_stride(S) * (size_t)n);
    const size_t start4 = align256(sizeof(double) * 4 * (size_t)n);
    const size_t total = nd * n_double_arrays + ni * n_int_arrays + partials + 2 * hist + selcnt + align256(sizeof(FitScalars)) + kQueueBytes + kBarrierBytes + kPlaceWords * 8 + nfbytes + rowpack + start4 + align256(sizeof(unsigned int) * kSfWorkWords);
    hipError_t e = hipMalloc(&c->ws, total);
    if (e != hipSuccess) return fail(c, CHICDIFF_E_NOMEM, "workspace of %zu bytes: %s", total, hipGetErrorString(e));
    c->ws_bytes = total;
    char *p = (char *)c->ws;
    auto takeD = [&](double *&ptr) { ptr = (double *)p; p += nd; };
    auto takeI = [&](int32_t *&ptr) { ptr = (int32_t *)p; p += ni; };
    FitWork &w = c->w;
    takeD(w.baseMean); takeD(w.baseVar); takeD(w.gm0); takeD(w.gm1); takeD(w.rough); takeD(w.binit0); takeD(w.binit1);
    takeD(w.crow); takeD(w.dispGene); takeD(w.dispFit); takeD(w.dispMAP); takeD(w.disp); takeD(w.beta0); takeD(w.beta1);
    takeD(w.resid);
    takeI(w.allZero); takeI(w.geneIter); takeI(w.mapIter); takeI(w.outlier); takeI(w.betaIter); takeI(w.optimConv);
    takeI(w.order);
    { int32_t *q; takeI(q); w.cls = (uint8_t *)q; }
    takeI(w.gridlist);
    w.partials = (double *)p; p += partials;
    w.hist = (double *)p; p += hist;
    w.hist_local = (double *)p; p += hist;
    w.selcnt = (double *)p; p += selcnt;
    w.sc = (FitScalars *)p; p += align256(sizeof(FitScalars));
    w.logfact = c->d_logfact;
    w.queue = (unsigned long long *)p; p += kQueueBytes;
    w.barrier = (unsigned int *)p; p += 1024;
    w.xchg = (unsigned long long *)p; p += kXchgBytes;
    w.place = (unsigned long long *)p; p += kPlaceWords * 8;
    c->d_nf_tmp = (double *)p; p += nfbytes;
    w.rowpack = p; p += rowpack;
    w.start = (double *)p; p += start4;
    c->d_sfhist = (unsigned int *)p;
    c->sfhist_dirty = true;  // (cleared by the first select that uses it)
    c->cap_n = n;
    c->cap_S = S;
    // scalars, queue heads and barrier counters start from zero: size_factors_impl runs before any fit has cleared them, and a
    // garbage sel_overflow there would send ONE rank of a sharded call into a second pass its peers do not make
    HIPCHK(c, hipMemsetAsync(w.sc, 0, align256(sizeof(FitScalars)) + kQueueBytes + kBarrierBytes, c->stream));
    return CHICDIFF_OK;
}

// The context's grow-only buffers (device | pinned): *p holds *have units of `unit` bytes; one that is too small for `want` is freed
// — after the stream's work, which may still use it, where `sync` says so — and allocated anew.  The words of fmt name it in the
// message of a failure, which returns `code`.
static int grow(chicdiff_hip_ctx *c, bool pinned, void **p, size_t *have, size_t want, size_t unit, bool sync, int code, const char *fmt, va_list ap) {
    if (*have >= want) return CHICDIFF_OK;
    if (*p) {
        if (sync) HIPCHK(c, hipStreamSynchronize(c->stream));
        (void)(pinned ? hipHostFree(*p) : hipFree(*p));
        *p = nullptr;
        *have = 0;
    }
    const hipError_t e = pinned ? hipHostMalloc(p, want * unit) : hipMalloc(p, want * unit);
    if (e != hipSuccess) {
        char words[384];
        vsnprintf(words, sizeof words, fmt, ap);
        return fail(c, code, "%s: %s", words, hipGetErrorString(e));
    }
    *have = want;
    return CHICDIFF_OK;
}
int cd::grow_dev(chicdiff_hip_ctx *c, void **p, size_t *have, size_t want, size_t unit, bool sync, int code, const char *fmt, ...) {
    va_list ap;
    va_start(ap, fmt);
    const int rc = grow(c, false, p, have, want, unit, sync, code, fmt, ap);
    va_end(ap);
    return rc;
}
int cd::grow_pin(chicdiff_hip_ctx *c, void **p, size_t *have, size_t want, size_t unit, bool sync, int code, const char *fmt, ...) {
    va_list ap;
    va_start(ap, fmt);
    const int rc = grow(c, true, p, have, want, unit, sync, code, fmt, ap);
    va_end(ap);
    return rc;
}

int cd::ensure_aux(chicdiff_hip_ctx *c, size_t bytes) {
    return grow_dev(c, (void **)&c->aux, &c->aux_bytes, bytes, 1, true, CHICDIFF_E_NOMEM, "scratch of %zu bytes", bytes);
}
// the host-buffer entry points' device arena and pinned staging area
int cd::ensure_io(chicdiff_hip_ctx *c, size_t dev_bytes, size_t pin_bytes) {
    if (int rc = grow_dev(c, (void **)&c->io_dev, &c->io_dev_bytes, dev_bytes, 1, true, CHICDIFF_E_NOMEM, "device arena of %zu bytes", dev_bytes)) return rc;
    return grow_pin(c, (void **)&c->io_pin, &c->io_pin_bytes, pin_bytes, 1, true, CHICDIFF_E_NOMEM, "pinned staging of %zu bytes", pin_bytes);
}

// with timing on (mode 1), every collective gets an event pair of its own, whatever scope it sits in: "allreduce" / "allgather" in
// chicdiff_hip_kernel_times = number of collectives of the call, their summed duration on the stream and the bytes this rank
// handed over (that time is ALSO inside the enclosing scope's figure — size_factors, trend_fit, mad_select — so it is a
// breakdown, not an extra term)
struct CollTimer {
    chicdiff_hip_ctx *c;
    int idx = -1;
    hipEvent_t e0 = nullptr, e1 = nullptr;
    __attribute__((noinline)) CollTimer(chicdiff_hip_ctx *c_, const char *name, double bytes) : c(c_) {  // out of line: off do_allreduce's own path
        if (c->timing != 1) return;
        idx = timer_slot(c, name);
        c->timers[idx].bytes += bytes;
        e0 = take_event(c);
        e1 = take_event(c);
        (void)hipEventRecord(e0, c->stream);
    }
    ~CollTimer() {
        if (idx < 0) return;
        (void)hipEventRecord(e1, c->stream);
        c->pending.push_back({idx, e0});
        c->pending.push_back({idx, e1});
    }
};

int cd::do_allreduce(chicdiff_hip_ctx *c, double *dev, int64_t count) {
    if (!c->allreduce) return CHICDIFF_OK;  // a callback registered with world_size 1 is still called (tests)
    int rc;
    {
        CollTimer t(c, "allreduce", 8.0 * (double)count);
        rc = c->allreduce(c->allreduce_user, dev, count);
    }
    if (rc != 0) return rc == kCollMsgSet && c->allreduce == rccl_allreduce_cb ? CHICDIFF_E_COMM : fail(c, CHICDIFF_E_COMM, "all-reduce callback failed");
    return CHICDIFF_OK;
}
// every rank contributes `count` doubles at `send`; `recv` gets world x count, rank r's block at r * count
int cd::do_allgather(chicdiff_hip_ctx *c, const double *send, double *recv, int64_t count) {
    int rc;
    {
        CollTimer t(c, "allgather", 8.0 * (double)count);
        rc = c->allgather(c->allgather_user, send, recv, count);
    }
    if (rc != 0) return rc == kCollMsgSet && c->allgather == rccl_allgather_cb ? CHICDIFF_E_COMM : fail(c, CHICDIFF_E_COMM, "all-gather callback failed");
    return CHICDIFF_OK;
}

// ---- device memory for hosts without their own GPU arrays (the R shim) ---------------------------------------
extern "C" int chicdiff_hip_malloc(chicdiff_hip_ctx *c, uint64_t bytes, void **d_ptr) {
    if (!c || !d_ptr) return CHICDIFF_E_INVALID;
    *d_ptr = nullptr;
    HIPCHK(c, hipSetDevice(c->device));
    hipError_t e = hipMalloc(d_ptr, bytes ? (size_t)bytes : 1);
    if (e != hipSuccess) return fail(c, CHICDIFF_E_NOMEM, "device allocation of %llu bytes: %s", (unsigned long long)bytes, hipGetErrorString(e));
    std::lock_guard<std::mutex> lock(c->user_mu);
    c->user_allocs.insert(*d_ptr);
    return CHICDIFF_OK;
}
extern "C" int chicdiff_hip_free(chicdiff_hip_ctx *c, void *d_ptr) {
    if (!c) return CHICDIFF_E_INVALID;
    if (!d_ptr) return CHICDIFF_OK;
    {
        std::lock_guard<std::mutex> lock(c->user_mu);
        if (!c->user_allocs.erase(d_ptr)) return fail(c, CHICDIFF_E_INVALID, "chicdiff_hip_free: not an allocation of this context (or freed already)");
    }
    HIPCHK(c, hipSetDevice(c->device));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    HIPCHK(c, hipFree(d_ptr));
    return CHICDIFF_OK;
}
extern "C" int64_t chicdiff_hip_outstanding_allocations(chicdiff_hip_ctx *c) {
    if (!c) return -1;
    std::lock_guard<std::mutex> lock(c->user_mu);
    return (int64_t)c->user_allocs.size();
}
extern "C" int chicdiff_hip_memcpy_h2d(chicdiff_hip_ctx *c, void *d_dst, const void *h_src, uint64_t bytes) {
    if (!c || (bytes && (!d_dst || !h_src))) return c ? fail(c, CHICDIFF_E_INVALID, "memcpy_h2d: NULL pointer") : CHICDIFF_E_INVALID;
    HIPCHK(c, hipSetDevice(c->device));
    HIPCHK(c, hipMemcpyAsync(d_dst, h_src, (size_t)bytes, hipMemcpyHostToDevice, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    return CHICDIFF_OK;
}
extern "C" int chicdiff_hip_memcpy_d2h(chicdiff_hip_ctx *c, void *h_dst, const void *d_src, uint64_t bytes) {
    if (!c || (bytes && (!h_dst || !d_src))) return c ? fail(c, CHICDIFF_E_INVALID, "memcpy_d2h: NULL pointer") : CHICDIFF_E_INVALID;
    HIPCHK(c, hipSetDevice(c->device));
    HIPCHK(c, hipMemcpyAsync(h_dst, d_src, (size_t)bytes, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    return CHICDIFF_OK;
}
