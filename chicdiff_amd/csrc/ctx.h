// ctx.h — what the host sources of include/chicdiff_hip.h share (ctx.hip, fit_api.hip, stage_api.hip, text_api.hip, table_api.hip, selftest_api.hip):
// the context, its options and timers, and the helpers that more than one of them calls.  Host translation units only: no
// *_kernels.hip file and no header that one of them includes may include it.
#pragma once
#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <algorithm>
#include <mutex>
#include <string>
#include <vector>
#include <unordered_set>

#include "chinput.h"
#include "common.h"
#include "prior_mc.h"

using namespace cd;

struct KTimer {
    std::string name;
    hipEvent_t e0 = nullptr, e1 = nullptr;
    double ms = 0;
    int launches = 0;
    double bytes = 0;  // collectives: payload this rank handed to the transport
};

// options only the host reads (chicdiff_hip_set_option; the others are the tuning tail of cd::Opts); the defaults are what the benchmarks run
struct HostOpts {
    int select_all_rounds = 0;
    int trend_one_launch_per_pass = 0;
    int sharded_trend_gather = 1;  // sharded fits: gather the rows of the trend on every rank (two collectives) instead of one all-reduce per IRLS pass
    int trend_mad_in_kernel = 1;   // the persistent trend kernel also takes the median / MAD of the residuals (0: separate launches)
    int local_trend_substitute = 1;  // 0: a failed parametric trend is reported (CHICDIFF_ST_TREND_FAILED), not replaced by the local fit
    int fuse_offsets = 1;  // 0 = offsets always as a launch of their own, 2 = always inside prep: the bit-identity test
    int prep_blocks = 0;   // test handle: at most this many workgroups for prep16_kernel (0 = one resident round), so that small fits run several tiles per workgroup
    int theta_grid_concurrency = 5;  // theta grid: fits in flight at once (1 = one after the other)
    int host_copy_threads = 12;      // host threads that move caller buffers to / from the pinned staging area
    // bench hook (a 1-rank communicator only): the trend's rows are gathered as if N ranks had each sent this rank's block — the
    // single-launch trend + MAD kernel then runs on N x n rows, which is what EVERY rank of an N-GPU fit does (bench.py's rehearsal
    // of a rank's step at its share of the rows; the coefficients are those of the n rows up to rounding)
    int bench_fake_world = 0;
    // test hook (one-shot bits, consumed by the next call that reaches the step): 1 = this rank's fit reports a select candidate-list
    // overflow, 2 = this rank's persistent trend kernel reports a grid-barrier timeout, 4 = this rank's size-factor select reports an
    // overflow.  Each verdict is all-reduced, so every rank of a sharded fit must re-enter together.
    int fault_inject = 0;
    int region_assemble_generic = 0;  // test option: every tile of region_assemble takes the generic path
    int table_write_half_kib = 0;  // test handle: bytes (KiB) of one half of the pinned area in chicdiff_hip_table_write_dev (0: up to 64 MiB)
    int chicago_tables_run_merge = 1;  // chicago_tables: runs of rows with one slot are merged inside the wave before the global atomic
    int sf_log_table = 1;  // size factors, direct route: log k of a count below kSfLogK from a table in LDS (0: a table logarithm per count)
    int wald_final_row_constant = 1;  // wald_final: sum_j y_j log(alpha mu_j) of a row the IRLS converged on from wald_prep's row constant (0: a table logarithm per sample)
};

struct chicdiff_hip_ctx {
    int device = 0;
    bool no_persistent_trend = false;  // set after a grid-barrier timeout (see fit_dev_impl)
    // tuning / test options (chicdiff_hip_set_option, the only writer): `tune` is what make_opts starts from, its tuning tail
    // (spread .. mad_value_cap) is the storage of those options
    Opts tune{};
    HostOpts host;
    char *tg_buf = nullptr;    // ... the gathered rows (grow-only)
    size_t tg_bytes = 0;
    double shard_n[kSelMaxWorld] = {0};  // rows of every rank's shard, exchanged with the argument verdicts at the start of a sharded call
    bool shard_n_valid = false;
    // set by gathered_trend for the rest of the fit: the whole fit's (baseMean, dispGeneEst) rows are on this rank
    int64_t tg_total = 0;
    double *tg_x = nullptr, *tg_y = nullptr, *tg_resid = nullptr;
    int32_t *tg_flags = nullptr;
    int32_t *h_flag = nullptr;  // pinned: sel_overflow of the size-factor select (read with the call's last synchronisation)
    // set by an entry point for the fit it is about to make (d_nf = d_nf_tmp): the offsets are formed from FullMean inside the fit's
    // first kernel instead of by a launch of their own (common.h FusedOffsets); cleared when the fit returns
    FusedOffsets fuse;
    int refits = 0;               // refits the last call went through (select overflow / barrier timeout / local substitute), for the tests
    bool sf_overflow_seen = false;  // fit_dev_impl: some rank's size-factor select (run by the caller just before) overflowed
    int32_t *d_carry = nullptr;   // device word that survives the fit's clearing of its scalars: sel_overflow of the size-factor select
    // host-buffer entry point: device arena + pinned staging, both grow-only (no allocation per call once warm)
    char *io_dev = nullptr, *io_pin = nullptr;
    size_t io_dev_bytes = 0, io_pin_bytes = 0;
    ChinputCols *chin = nullptr;            // columns of the .chinput file read last (chicdiff_hip_chinput_read)
    // chicdiff_hip_chinput_read_dev: the body's text and the three columns on the device (grow-only, apart from aux and the io arena:
    // chicdiff_hip_count_table_dev's workspace must not overwrite the columns), and the two halves of the pinned staging area
    char *chin_text = nullptr, *chin_pin = nullptr;
    int32_t *chin_cols = nullptr;
    size_t chin_text_bytes = 0, chin_pin_half = 0, chin_cols_rows = 0;
    hipEvent_t chin_ev[2] = {nullptr, nullptr};
    int64_t chin_dev_rows = -1;             // >= 0: the read that came last was a device read of this many rows (chin_cols holds them)
    // chicdiff_hip_peaks_read_dev: the columns of the peak matrix read last (grow-only, apart from every workspace; the text goes
    // through chin_text / chin_pin): (6, pk_stride) int32, dist, (pk_nscore, pk_stride) scores, line offsets
    char *pk_buf = nullptr;
    size_t pk_buf_bytes = 0;
    int64_t pk_stride = 0, pk_rows = -1;    // pk_rows >= 0: a successful read of this many rows
    int pk_nscore = 0;
    // while chin_text still holds the body of that read (chicdiff_hip_peaks_textkeys_dev walks it): its length and separator
    int64_t pk_text_bytes = -1;
    int pk_sep = 0;
    // chicdiff_hip_table_write_dev: the table's text on the device (grow-only); it leaves through chin_pin / chin_ev
    char *tt_text = nullptr;
    size_t tt_text_bytes = 0;
    // host-buffer entry point: columns that are final once the MAP dispersions exist leave for the host on a second
    // stream while the Wald stage runs (set for the duration of one chicdiff_hip_nbglm_fit call)
    struct EarlyCopy {
        int n = 0;
        struct Item { int col; char *pin; size_t bytes; } item[10];  // col: 0 baseMean 1 baseVar 2 dispGeneEst 3 dispFit 4 dispMAP 5 dispersion 6 dispGeneIter 7 dispIter 8 dispOutlier 9 allZero
        hipEvent_t ready = nullptr, done = nullptr;
        bool issued = false;
    } *early = nullptr;
    hipStream_t copy_stream = nullptr;      // also the second stream of the independent-filtering sorts
    hipEvent_t ev_fork = nullptr, ev_join = nullptr;
    std::vector<chicdiff_hip_ctx *> lanes;  // theta grid: child contexts (own stream + workspace), one per concurrent fit
    int cu_count = 0;  // compute units of the device (the persistent trend kernel needs one resident workgroup per CU it launches)
    hipStream_t own_stream = nullptr, stream = nullptr;
    chicdiff_allreduce_fn allreduce = nullptr;
    void *allreduce_user = nullptr;
    chicdiff_allgather_fn allgather = nullptr;  // optional: without it the trend rows are gathered by a sum-all-reduce over zero-filled arrays
    void *allgather_user = nullptr;
    int world = 1, rank = 0;
    // direct RCCL path (chicdiff_hip_rccl_init): librccl is dlopen'ed, never linked
    void *rccl_lib = nullptr, *rccl_comm = nullptr;
    int (*rccl_allreduce)(const void *, void *, size_t, int, int, void *, hipStream_t) = nullptr;
    int (*rccl_allgather)(const void *, void *, size_t, int, void *, hipStream_t) = nullptr;
    int (*rccl_comm_destroy)(void *) = nullptr;
    const char *(*rccl_error_string)(int) = nullptr;
    char err[512] = {0};
    // workspace
    int64_t cap_n = 0;
    int cap_S = 0;
    void *ws = nullptr;
    size_t ws_bytes = 0;
    char *aux = nullptr;  // scratch of the post-processing entry points (sort / scan temporaries)
    size_t aux_bytes = 0;
    FitWork w{};
    double *d_sf = nullptr;   // kMaxS doubles
    double *d_logfact = nullptr;  // kLogFactN doubles: log(k!) (wald_prep)
    PmcTable *d_pmc[4] = {nullptr, nullptr, nullptr, nullptr};  // simulated residual densities + loess operator per d.f. (prior_mc.h)
    double *d_nf_tmp = nullptr;
    unsigned int *d_sfhist = nullptr;  // kSfWorkWords: value-bin histograms (+ list lengths) of the direct size-factor select; zero between calls (sf_pick_kernel)
    bool sfhist_dirty = false;         // ... unless a call's launches did not all go out
    FitScalars *h_sc = nullptr;  // pinned
    double *h_sf = nullptr;      // pinned, kMaxS
    // timing
    int timing = 0;  // 0 off, 1 every stage, 2 the three fit kernels only (disp_gene, disp_map, wald_irls)
    std::vector<KTimer> timers;
    std::vector<std::pair<int, hipEvent_t>> pending;
    std::vector<hipEvent_t> event_pool;  // recycled: creating events per launch cost ~0.9 ms per step
    int scope_depth = 0;                 // nested scopes are folded into the outermost one
    // chicdiff_hip_malloc: the caller's device vectors, so that destroying the context releases what its host forgot or could not
    // release any more (R runs the finalizers of one garbage collection in no particular order: a context can go before its vectors)
    std::unordered_set<void *> user_allocs;
    std::mutex user_mu;
};

namespace cd {

// once per process, defined in ctx.hip: the message of a failed chicdiff_hip_create (chicdiff_hip_last_error(NULL)), and the
// simulated residual densities + loess operator of one d.f. (prior_mc.h)
extern char g_create_err[512];
const PmcTable &pmc_table(int df);

int fail(chicdiff_hip_ctx *c, int code, const char *fmt, ...);
inline size_t align256(size_t x) { return (x + 255) & ~(size_t)255; }

// ctx.hip
void timing_reset(chicdiff_hip_ctx *c);
void timing_collect(chicdiff_hip_ctx *c);
int timer_slot(chicdiff_hip_ctx *c, const char *name);  // index in c->timers of the timer called `name`, added if new
hipEvent_t take_event(chicdiff_hip_ctx *c);             // from c->event_pool, or a new one
int grow_dev(chicdiff_hip_ctx *c, void **p, size_t *have, size_t want, size_t unit, bool sync, int code, const char *fmt, ...);
int grow_pin(chicdiff_hip_ctx *c, void **p, size_t *have, size_t want, size_t unit, bool sync, int code, const char *fmt, ...);
int ensure_workspace(chicdiff_hip_ctx *c, int64_t n, int S);
int ensure_aux(chicdiff_hip_ctx *c, size_t bytes);
int ensure_io(chicdiff_hip_ctx *c, size_t dev_bytes, size_t pin_bytes);
int do_allreduce(chicdiff_hip_ctx *c, double *dev, int64_t count);
int do_allgather(chicdiff_hip_ctx *c, const double *send, double *recv, int64_t count);
// fit_api.hip
int check_counts_group(chicdiff_hip_ctx *c, int64_t n, int32_t S, const int32_t *group, FitDims &d);
int check_opts(chicdiff_hip_ctx *c, const chicdiff_nbglm_opts *opts);
Opts make_opts(const chicdiff_hip_ctx *c, const chicdiff_nbglm_opts *in, int S);
struct LfTree {  // the local trend's vertices as the host grows them (local_trend_fit)
    int nv = 0;
    double x[kLfMaxV], h[kLfMaxV], f[kLfMaxV], d[kLfMaxV];
};
int global_stage(chicdiff_hip_ctx *c, FitDims d, const Opts &o, bool all_rounds, LfTree *tree);
bool substitute_local_trend(const chicdiff_hip_ctx *c, const Opts &o);  // the verdict of fit_dev_impl on a failed parametric trend
bool prior_by_simulation(const FitDims &d, const Opts &o);
double *resid_hist_of(const FitWork &w);  // the 40 device doubles prior_mc counts the residuals into

}  // namespace cd

#define HIPCHK(c, call)                                                                              \
    do {                                                                                             \
        hipError_t e_ = (call);                                                                      \
        if (e_ != hipSuccess) return fail(c, CHICDIFF_E_HIP, "%s: %s", #call, hipGetErrorString(e_)); \
    } while (0)

// ---- timing: one event pair per launch, accumulated per kernel name when the call ends (timing_collect) ------
struct Scope {
    chicdiff_hip_ctx *c;
    int idx = -1;
    hipEvent_t e0 = nullptr, e1 = nullptr;
    Scope(chicdiff_hip_ctx *c_, const char *name) : c(c_) {
        if (!c->timing) return;
        if (c->scope_depth++ > 0) return;  // inside an outer scope: no events of its own
        // mode 2: an event pair costs ~2 us on the stream and as much on the host when it is read back; a caller that times whole
        // calls (bench.py) brackets only the fit kernels — 0.09 ms less per call than bracketing all ~20 stages
        if (c->timing == 2 && strcmp(name, "disp_gene") != 0 && strcmp(name, "disp_map") != 0 && strcmp(name, "wald_irls") != 0) return;
        // mode 3: the gene-wise line search alone — the dominant kernel of every configuration measured (an event on the stream is a
        // packet of its own: each pair costs ~12 us of a 1.3 ms step at 250 k rows; rocprofv3 kernel trace, profiles/r05_kernel_gaps_*)
        if (c->timing == 3 && strcmp(name, "disp_gene") != 0) return;
        idx = timer_slot(c, name);
        e0 = take_event(c);
        e1 = take_event(c);
        (void)hipEventRecord(e0, c->stream);
    }
    ~Scope() {
        if (!c->timing) return;
        c->scope_depth--;
        if (idx < 0) return;
        (void)hipEventRecord(e1, c->stream);
        c->pending.push_back({idx, e0});
        c->pending.push_back({idx, e1});
    }
};
