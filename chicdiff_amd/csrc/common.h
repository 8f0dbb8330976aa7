// common.h — shared declarations of the HIP implementation behind include/chicdiff_hip.h.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/chicdiff_hip.h"
#include "fit_driver.h"
#include "fit_state.h"

namespace cd {

constexpr int kRedBlocks = 1024;   // fixed grid of the reduction passes (deterministic two-stage sums)

struct FitDims {
    int64_t n;
    int32_t S, p, nA, nB;
    uint64_t gmask;  // bit j set = sample j in group B
};

// workspace pointers of one fit (all device memory, length n unless noted)
struct FitWork {
    double *baseMean, *baseVar, *gm0, *gm1, *rough, *binit0, *binit1, *crow;
    double *dispGene, *dispFit, *dispMAP, *disp, *beta0, *beta1, *resid;
    int32_t *allZero, *geneIter, *mapIter, *outlier, *betaIter, *optimConv;
    int32_t *order;               // schedule of the gene-wise line search: row indices, likely-long rows first (disp_kernels.hip)
    uint8_t *cls;                 // ... and the class each row was put in (255 = all-zero row: not scheduled)
    int32_t *gridlist;            // rows whose dispersion line search did not converge (fitDispGrid runs in disp_grid_kernel); their number: queue[16] gene-wise, queue[24] MAP
    char *rowpack;                // row-major copy of the fit's inputs, row i at rowpack + i * row_stride(S): a 32-byte header (kRowHdr), nf[S]
                                  // doubles, counts[S] int32 (written by prep): the row-queue kernels visit rows out of order, and a row that
                                  // is 32 + 12 S contiguous bytes costs one or two cache lines instead of 2 S + 4
    double *start;                // 4 doubles per row, dense: what the kernel that visits the rows next needs besides the record — gene-wise
                                  // search: alpha_init, log alpha_init; MAP search: start value, prior mean; IRLS: alpha, row constant of the
                                  // deviance, the two start values.  (Rounds 3-4 kept them in the second half of the record's header: 16-byte
                                  // stores 128 bytes apart, which cost disp_init 50 of its 74 us at 2 M rows.)
    double *partials;             // kRedBlocks x 72 doubles
    double *hist;                 // kMaxS*2 x kSelBins doubles (f64 so it can ride the all-reduce)
    double *hist_local;           // same size: this rank's round-2 histogram, kept aside for the sharded shortcut
    double *selcnt;               // kSelMaxWorld x kMaxS*2 doubles: per-rank candidate counts
    unsigned long long *queue;    // work-queue heads (kQueueBytes): [0] gene-wise, [1] MAP, [8..15] spare, [16] / [24] lengths of the gene-wise / MAP grid lists, [32 + 8 h] the IRLS's eight heads, 64 bytes apart, [192 + 8 h] the MAP line search's; [104], [112]: role counters of the gene-wise launch's filler waves (kRoleFront, kRoleFill)
    unsigned long long *place;    // kPlaceWords words: where the waves of a gene-wise launch with fillers landed, one word per compute unit; zeroed by disp_init when such a launch follows
    unsigned int *barrier;        // 9 x 64 B: grid-barrier counters of the persistent trend kernel
    unsigned long long *xchg;     // kXchgBytes behind them: the self-tagged words of its passes' partial sums (trend_kernels.hip, "exchange"); zeroed with the counters at the head of every fit
    FitScalars *sc;
    const double *logfact;        // log(k!) for k < kLogFactN
};
// the fixed-order sums of a reduction pass sit behind the block partials: 128 doubles (the trend's sums first; from + 32 the
// residual histogram of the simulated prior, ctx.h resid_hist_of).  By value, as the kernels take it: with a reference to their
// argument, trend_reduce_kernel and trend_step_kernel compile to other code (tools/device_code_diff.py)
__host__ __device__ inline double *sums_of(FitWork w) { return w.partials + (size_t)kRedBlocks * 72; }
constexpr int kLogFactN = 1024;
constexpr int kQueueBytes = 2048;  // FitWork::queue
constexpr int kXchgBytes = 2 * 16 * 256 * 16;            // FitWork::xchg: [pass parity][16 sums][256 workgroups][2 words]
constexpr int kBarrierBytes = 1024 + kXchgBytes;         // FitWork::barrier and FitWork::xchg: what a fit's first fill clears behind the scalars and the queue heads
// ---- filler waves of the gene-wise line search (disp_kernels.hip, "front waves and fillers") ----
constexpr int kPlaceWords = 2048;  // FitWork::place[cu]: one word per compute unit (XCC, SE, SH, CU ids of HW_ID), arrivals per SIMD in its four 16-bit fields
constexpr int kRoleFront = 104, kRoleFill = 112;     // queue[104] / queue[112] (cache lines of their own): waves that took a front index / asked to be a filler so far
// The two-ended queue.  One 64-bit word counts the claims from the head (low half, f) and from the end (high half, b); a claim is one
// atomic add of kClaimFront or kClaimBack, and `old` is what it returned.  The claim is valid exactly while f + b < chunks — every atomic
// raises f + b by one, so the valid claims are the first `chunks` atomics, whoever makes them — and then names chunk f (from the head)
// or chunks - 1 - b (from the end): disjoint, and together every chunk once.  A valid claim is always worked by the wave that made it.
constexpr unsigned long long kClaimFront = 1ull, kClaimBack = 1ull << 32;
__host__ __device__ inline bool queue_claim(unsigned long long old, bool back, uint32_t chunks, uint32_t &chunk) {
    const uint32_t f = (uint32_t)old, b = (uint32_t)(old >> 32);
    chunk = back ? chunks - 1u - b : f;
    return f < chunks && b < chunks - f;  // f + b < chunks, in 32-bit compares (the scalar unit has no ordered 64-bit one)
}
// Whether a filler may claim (again).  `old` is the word its last claim returned, `claimed` whether it has made one (before the first
// claim it has seen nothing, and only the launch-wide facts count).  It stops for good once its last chunk was the boundary chunk or
// in front of it — first_back is the first chunk that lies wholly inside the rows that cannot be long; first_back >= chunks: there is
// none — or once the front counter it saw has reached stop_f (the set share of the front's own chunks; 0 = fillers never claim,
// 0xffffffff = no such stop).  So fillers overshoot the boundary by at most one chunk per wave, and nothing ever waits.
__host__ __device__ inline bool filler_claims(bool claimed, unsigned long long old, uint32_t chunks, uint32_t first_back, uint32_t stop_f) {
    if (first_back >= chunks || stop_f == 0u) return false;
    if (!claimed) return true;
    uint32_t chunk;
    if (!queue_claim(old, true, chunks, chunk)) return false;  // the queue is empty
    return chunk > first_back && (uint32_t)old < stop_f;
}
// stop_f from the option's percentage: share of the front's own chunks [0, first_back)
__host__ __device__ inline uint32_t filler_stop_f(int percent, uint32_t chunks, uint32_t first_back) {
    if (percent >= 100) return 0xffffffffu;
    if (percent <= 0) return 0u;
    const uint32_t own = first_back < chunks ? first_back : chunks;
    return (uint32_t)(((unsigned long long)own * (unsigned)percent + 99ull) / 100ull);
}
// bytes between rows of FitWork::rowpack: 12 S rounded up so that a row never straddles more 128-byte lines than it must
constexpr int kRowHdr = 32;  // four doubles in front of every row: group mean A (its sign bit set: the row is all zero), group mean B, two
                             // spare (the per-stage start values moved to FitWork::start)
__host__ __device__ inline int64_t row_stride(int S) {
    const int64_t bytes = kRowHdr + (int64_t)S * 12;
    return bytes <= 64 ? 64 : (bytes + 127) / 128 * 128;
}
__device__ __forceinline__ double *row_hdr(char *rowpack, int64_t r, int S) { return reinterpret_cast<double *>(rowpack + r * row_stride(S)); }

struct Opts {
    double minDisp, dispTol, kappa0, betaTol, minmu, outlierSD, dispPriorVarIn, maxDisp, trendIn[2];
    int32_t maxit, betaMaxit;
    int32_t fit_type = 0;  // 0 parametric trend, 1 mean (chicdiff_nbglm_opts.fitType)
    // tuning (chicdiff_hip_set_option; the context's `tune` is their storage): not part of the algorithm, results do not depend on them
    int32_t spread = 1;     // line search: samples-across-lanes evaluation for straggler waves (0 = row per lane only)
    int32_t min_waves = 0;  // line search: waves per SIMD (2 .. 4; 0 = by launch_disp's rule)
    int32_t schedule = 1;   // gene-wise line search / IRLS: visit the rows likely-long first (0 = natural order; gene-wise only: 3 = the six
                            // half-decade classes of rounds 3-6, 4 = minDisp starts last instead of in front of the score >= 3.16 rows; 2 is not a mode)
    int32_t deal = 0;       // ... entries per group of its static deal (0 = chosen from the number of entries per wave)
    int32_t chunk = 0;      // line search: rows per dequeue (0 = chosen from the row count; 8 .. 64)
    int32_t classes_a = 0;  // gene-wise line search: score classes dealt out statically (0 = the default, 2; 1 .. 6)
    int32_t xim_here = 0;   // (set by the fit driver, not an option) single rank: disp_init forms xim from the column sums itself, no xim_kernel launch
    int32_t prio = 0;       // line search: issue priority by search age, one level per `prio` iterations (0 = off); option "line_search_prio"
    int32_t fillers = -1;   // gene-wise line search: a third wave per SIMD at priority 0 that takes only rows which cannot be long (0 off, 1 on, -1 = by launch_disp's rule); option "line_search_fillers"
    int32_t filler_stop = -1;  // ... fillers stop claiming once the front waves have claimed this share (percent) of their own chunks (100 = never, -1 = kFillerStopDefault); option "line_search_filler_stop"
    int32_t trend_blocks = 0;  // persistent trend kernel: at most this many workgroups (0 = one per CU); option "trend_persistent_blocks"
    int32_t trend_speculate = 1;  // persistent trend kernel: passes announced by fit_state.h trend_step_spec also sum the next glm() call's start pass; option "trend_speculate"
    int32_t trend_exchange = 1;   // ... its passes' partial sums travel as self-tagged words, no grid barrier per pass (0 = publish, grid barrier, re-read); option "trend_exchange"
    int32_t mad_route = 1;        // ... its MAD step: 1 = value-binned select (three grid barriers), 0 = two radix selects (six); option "mad_select_route"
    int32_t mad_value_cap = 0;    // ... keys a candidate list of the value-binned select may hold (0 = kVbCap); test hook, option "mad_value_cap"
};

// ---- schedule of a row-queue kernel (disp_kernels.hip order_*): rows in class order; the class counts per tile of rows come from
// the kernel that writes the classes (disp_init for the gene-wise search; wald_prep, for fits of one row per thread, for the IRLS)
constexpr int kSchedClasses = 6, kSchedBlocks = 1024;  // (the IRLS's class count: wald_prep uses four of them)
inline void order_tiles(int64_t n, int64_t &nblk, int64_t &tile) {
    nblk = (n + 255) / 256;
    if (nblk > kSchedBlocks) nblk = kSchedBlocks;
    tile = ((n + nblk - 1) / nblk + 255) / 256 * 256;
    nblk = (n + tile - 1) / tile;
}
// ---- classes of the gene-wise line search's schedule (disp_kernels.hip, "schedule of the gene-wise line search") ----
// The score alpha_init * (smaller group mean) ranks the rows by how likely they are to creep for all 100 iterations; the visit
// order follows it in steps of 1/8 decade from 0.0316 to 10 (the half-decade edges are the literals of the six-class order of
// rounds 3-6, so that order is the same partition, coarser).  Layout of the kSchedClassesFine = 23 class indices:
//    0       score < 0.0316
//    1 .. 16 the sixteen 1/8-decade steps up to 3.16      (0 .. 8: score < 0.316, the static deal "A" by default)
//   17       the rows that start at minDisp: never long (at most ~35 evaluations, mostly rejected steps), but longer than the rows
//            behind them (at most ~18), so the queue ends on those — empty under kSchedSix and kSchedMinDispLast
//   18 .. 21 the four steps from 3.16 to 10
//   22       score >= 10 (and the minDisp starts under kSchedSix and kSchedMinDispLast, where they were up to round 6)
// mode = Opts::schedule: kSchedSix (3) keeps the six-class order (its classes sit at indices 0, 5, 9, 13, 18, 22).
constexpr int kSchedClassesFine = 23, kSchedEdgesFine = 21, kSchedMinDispSlot = 17;
constexpr int kSchedSix = 3, kSchedMinDispLast = 4;  // values of Opts::schedule besides 0 (off) and 1 (on); 2 is not a mode
__host__ __device__ inline int sched_class(double a0, double gmin, double minDisp, int mode) {
    constexpr double edge[kSchedEdgesFine] = {0.0316, 0.0422, 0.0562, 0.0750, 0.1, 0.1334, 0.1778, 0.2371, 0.316, 0.4217, 0.5623,
                                              0.7499, 1.0, 1.3335, 1.7783, 2.3714, 3.16, 4.2170, 5.6234, 7.4989, 10.0};
    if (!(a0 > 1.5 * minDisp)) return (mode == kSchedSix || mode == kSchedMinDispLast) ? kSchedClassesFine - 1 : kSchedMinDispSlot;
    const double s = a0 * gmin;
    int f = 0;  // edges not above the score (a NaN score counts as the highest, as the chain of `s < edge` did)
    if (mode == kSchedSix) {
#pragma unroll
        for (int k = 4; k < kSchedEdgesFine; k += 4) f += !(s < edge[k]) ? 4 : 0;
        f += f > 0 ? 1 : 0;  // 0, 5, 9, 13, 17, 21: the first index of each half-decade
    } else {
#pragma unroll
        for (int k = 0; k < kSchedEdgesFine; k++) f += !(s < edge[k]) ? 1 : 0;
    }
    return f < kSchedMinDispSlot ? f : f + 1;
}
// first class index that is NOT dealt out statically when `a` of the six half-decade classes are (option "line_search_classes_a")
__host__ __device__ inline int sched_classes_a(int a, int mode) {
    if (a <= 0) return 0;
    if (a <= 3) return 1 + 4 * a;                                         // score < 0.1, 0.316, 1
    if (a == 4) return kSchedMinDispSlot;                                 // score < 3.16
    if (a == 5) return (mode == kSchedSix || mode == kSchedMinDispLast) ? kSchedClassesFine - 1 : kSchedMinDispSlot;  // all but the minDisp starts and what is behind them
    return kSchedClassesFine;
}
#ifdef __HIPCC__
// class counts per tile: hist[class * kSchedBlocks + block] (rows of fixed length: order_scatter_kernel reads them 16 bytes at a time)
// per-thread class counts -> hist (wave shuffles, then one LDS add per wave and class)
template <int NC>
__device__ __forceinline__ void order_hist_store(const unsigned int (&mine)[NC], unsigned int *hist) {
    __shared__ unsigned int s_cnt[NC];
    if (threadIdx.x < NC) s_cnt[threadIdx.x] = 0;
    __syncthreads();
#pragma unroll
    for (int k = 0; k < NC; k++) {
        unsigned int v = mine[k];
        for (int off = 32; off > 0; off >>= 1) v += __shfl_down(v, off);
        if ((threadIdx.x & 63) == 0 && v) atomicAdd(&s_cnt[k], v);
    }
    __syncthreads();
    if (threadIdx.x < NC) hist[threadIdx.x * kSchedBlocks + blockIdx.x] = s_cnt[threadIdx.x];
}
// the lanes of the wave that hold this lane's class (c < 32; a lane with valid == false has no peers): how many they are, and how many
// of them sit below this lane — five ballots whatever the number of classes
__device__ __forceinline__ void class_peers(int c, bool valid, int lane, unsigned int &rank, unsigned int &count) {
    unsigned long long m = __ballot(valid);
#pragma unroll
    for (int b = 0; b < 5; b++) {
        const bool bit = (c >> b) & 1;
        const unsigned long long set = __ballot(bit);
        m &= bit ? set : ~set;
    }
    rank = __popcll(m & ((1ull << lane) - 1ull));
    count = __popcll(m);
}
#endif

// ---- launchers (defined in the .hip files; all enqueue on `st` and never synchronise) -------
// disp_kernels.hip — prep, the gene-wise and MAP dispersion searches, their schedule
// fm != NULL (S <= 16): the offsets are formed here, from FullMean — sc(theta) of chicdiff.R:1635-1638 / M3 of :1583-1589, the very
// function offsets16_kernel runs — written to `nf` (the stages behind read them from there) and used at once: one read and one
// launch less than offsets + prep (round 5)
struct FusedOffsets { const double *fm = nullptr; const double *sf = nullptr; double theta = 0; int mix = 0; };
// -> the blocks whose partial column sums exist (launch_prep_finish's nblk); max_blocks > 0 caps the workgroups at S <= 16 (option "prep_blocks")
int launch_prep(const int32_t *counts, double *nf, FitDims d, FitWork w, Opts o, hipStream_t st, FusedOffsets fo = FusedOffsets(), int max_blocks = 0);
void launch_prep_finish(FitDims d, FitWork w, int nblk, double *slot, hipStream_t st);  // partials -> colsum, nnz (slot: as (hi, lo) pairs into this rank's slot instead)
void launch_xim(FitDims d, FitWork w, const double *slots, int world, hipStream_t st);  // (the ranks' slots ->) colsum -> xim
void launch_disp_gene(const int32_t *counts, const double *nf, FitDims d, FitWork w, Opts o, hipStream_t st);
void launch_order_build(FitDims d, FitWork w, int classesA, bool have_hist, hipStream_t st, bool fine = false);  // w.cls -> w.order (schedule of a row-queue kernel; fine: kSchedClassesFine classes)
void launch_disp_map(const int32_t *counts, const double *nf, FitDims d, FitWork w, Opts o, hipStream_t st);
// trend_kernels.hip — dispersion trend, residuals and MAD, local fit, prior variance
// single rank (or the gathered rows of a sharded fit): whole trend fit, one launch; with_mad: the same launch goes on to the residuals,
// their median and MAD and the closed-form prior variance (w.resid, sc->med / nres / mad / varLogDispEsts / dispPriorVar)
void launch_trend_persistent(FitDims d, FitWork w, Opts o, hipStream_t st, bool with_mad);
int trend_persistent_blocks();  // workgroups that must be co-resident (grid barrier): needs that many CUs
void launch_trend_init(FitDims d, FitWork w, Opts o, hipStream_t st);
int trend_blocks();                                                       // grid of the trend pass = rows of 8 partial sums
void launch_trend_pass(FitDims d, FitWork w, Opts o, hipStream_t st, bool fused_step);  // pass (+ reduce + step when single rank)
void launch_trend_step(FitDims d, FitWork w, Opts o, hipStream_t st);   // fixed-order sum of the (all-reduced) partials + state machine step
constexpr int kLfMaxV = 100;  // locfit's maxk
struct LfVerts { int nv; int _pad; double x[kLfMaxV], f[kLfMaxV], d[kLfMaxV]; };  // vertices of the local trend, ascending x
void launch_lf_hist(FitDims d, FitWork w, Opts o, int use_dist, double xv, uint64_t prefix, int shift, double *hist, hipStream_t st);
void launch_lf_sums(FitDims d, FitWork w, Opts o, double xv, double h, double *partials, double *out8, hipStream_t st);
void launch_lf_eval(FitDims d, FitWork w, const LfVerts &v, hipStream_t st);
void launch_trend_gather(FitDims d, FitWork w, Opts o, double *xg, double *yg, hipStream_t st);
// all-gather transport of the sharded trend: rank r's block of `block` doubles holds x[maxn] | y[maxn] (its first off[r+1] - off[r]
// entries are rows); the copy below lays the ranks' rows out back to back
constexpr int kGatherMaxWorld = 64;
struct GatherLayout { int32_t world, _pad; int64_t block, maxn; int64_t off[kGatherMaxWorld + 1]; };
void launch_trend_compact(const GatherLayout &gl, const double *recv, double *xg, double *yg, hipStream_t st);
void launch_poke(int32_t *p, int32_t v, hipStream_t st);                       // *p = v on the stream (test hooks)
void launch_flag_to_double(const int32_t *flag, double *out, hipStream_t st);  // *out = *flag != 0 (a verdict on its way to a sum-all-reduce)
void launch_dispfit_resid(FitDims d, FitWork w, Opts o, hipStream_t st);
void launch_prior_var(FitDims d, FitWork w, Opts o, hipStream_t st);
void launch_resid_hist(FitDims d, FitWork w, double *out40, hipStream_t st);  // residual histogram for the d.f. <= 3 prior
void launch_prior_mc(FitDims d, FitWork w, const double *hist40, const void *table, hipStream_t st);  // simulation-matched prior variance
// wald_kernels.hip — the Wald stage and the fit's closing sums
void launch_wald_prep(const int32_t *counts, const double *nf, FitDims d, FitWork w, Opts o, hipStream_t st);
void launch_wald_irls(const int32_t *counts, const double *nf, FitDims d, FitWork w, Opts o, hipStream_t st);
// row_constant: sum_j y_j log(alpha mu_j) of a row the IRLS converged on from wald_prep's row constant (option "wald_final_row_constant")
void launch_wald_final(const int32_t *counts, const double *nf, FitDims d, FitWork w, Opts o, int row_constant,
                       const chicdiff_nbglm_out &out, hipStream_t st);
void launch_wald_intercept(const int32_t *counts, const double *nf, FitDims d, FitWork w, Opts o,
                           const chicdiff_nbglm_out &out, hipStream_t st);
// the fit's last kernel: deviance / row-count sums and this rank's verdicts into sc->final_sums, the size factors into sc->final_sf;
// carry: overflow flag of the size-factor select the caller ran before the fit (may be NULL); sf_dev: its size factors (may be NULL)
void launch_dev_sum_finish(FitDims d, FitWork w, const int32_t *carry, const double *sf_dev, hipStream_t st);

// global_kernels.hip — exact medians over all rows: radix select over keys produced on the fly; `mode` (SelMode, fit_driver.h) picks the
// key generator
struct SelArgs {
    int mode;
    int ncol;               // columns selected simultaneously (1, or S for size factors)
    int64_t n;
    const double *resid;    // SEL_RESID / SEL_ABSDEV: residuals (NaN = excluded)
    const double *ratio;    // SEL_SIZEFACTOR: log(count) - row log geometric mean, S x n (NaN = excluded)
    int S;
    int shift;              // bit position of the current digit
    double *sf_out;         // SEL_SIZEFACTOR: where the size factors go as well (device, may be NULL)
    int32_t *overflow_out;  // sharded shortcut: set to 1 when a candidate list does not fit (NULL = sc->sel_overflow)
};
void launch_sel_hist(SelArgs a, FitWork w, hipStream_t st);     // digit histograms for the live prefixes
void launch_sel_step(SelArgs a, FitWork w, hipStream_t st);     // pick bins, extend prefixes
void launch_sel_shortcut(SelArgs a, FitWork w, hipStream_t st); // single rank: gather the candidates left after two rounds, finish by sorting
void launch_sel_finish(SelArgs a, FitWork w, hipStream_t st);   // prefixes -> values; median into sc
// sharded shortcut (fit_state.h): keep the local histogram, own count row, place candidates, sort + pick
void launch_sel_keep_local(SelArgs a, FitWork w, hipStream_t st);
void launch_sel_gather_counts(SelArgs a, FitWork w, int world, int rank, hipStream_t st);
void launch_sel_gather_place(SelArgs a, FitWork w, int world, int rank, hipStream_t st);
void launch_sel_gather_finish(SelArgs a, FitWork w, int world, int rank, hipStream_t st);

void launch_row_ratio(const int32_t *counts, int64_t n, int S, double *ratio, int32_t *clear_flag, hipStream_t st);  // keys of the size-factor medians (+ *clear_flag = 0)

// ---- direct select of the size-factor medians (global_kernels.hip, "size factors in two passes over the counts") ----
// The keys log(count) - row log geometric mean are never stored: a first pass over the counts bins them BY VALUE, a pick finds
// the bin(s) that hold the two middle ranks of every column, a second pass recomputes the keys and lists those of the picked bins,
// and a finish reads the exact order statistics off the lists.  Exactness asks two things of the bin function: that it never
// decreases as the key grows, and that both passes evaluate it alike — not that the bins be equally full or the ends open.
// Bins of equal width over [kSfBinLo, kSfBinLo + kSfBinSpan), the end bins taking whatever lies outside; as many bins per column
// as kSfHistWords LDS words allow for 4, 8 or 16 columns (3840, 1920, 960: bin width 1/480, 1/240, 1/120).
constexpr double kSfBinLo = -4.0, kSfBinSpan = 8.0;
constexpr int kSfHistWords = 15360;  // pass 1 keeps every column's histogram in LDS: 60 KB beside the 1 KB logarithm table
constexpr int kSfSubBins = 4096;     // the finish splits a picked bin's width once more
constexpr int kSfMaxS = 16;
constexpr int kSfWorkWords = kSfHistWords + 2 * kSfMaxS * 32;  // the global histograms, then the lists' lengths (one per 128 bytes)
__host__ __device__ inline int sf_bins(int S) { return kSfHistWords / (S <= 4 ? 4 : S <= 8 ? 8 : 16); }
__host__ __device__ inline double sf_bin_pos(double x, int nb) { return (x - kSfBinLo) * ((double)nb / kSfBinSpan); }
__host__ __device__ inline int sf_bin(double x, int nb) {
    const double u = floor(sf_bin_pos(x, nb));
    return u < 0.0 ? 0 : (u > (double)(nb - 1) ? nb - 1 : (int)u);
}
// ... and the sub-bin of a key inside bin b (keys of an end bin that lie outside the range all fall into the first / last one)
__host__ __device__ inline int sf_sub_bin(double x, int nb, int b) {
    const double u = floor((sf_bin_pos(x, nb) - (double)b) * (double)kSfSubBins);
    return u < 0.0 ? 0 : (u > (double)(kSfSubBins - 1) ? kSfSubBins - 1 : (int)u);
}
// hist: kSfWorkWords words, the histograms all zero (the pick leaves them so); lists: n x S words, column j's keys from j * n (free: the offsets buffer)
// cus: compute units of the device (both passes run one workgroup on each)
// log_table: both passes take log k of a count k < kSfLogK from a table the workgroup fills in LDS (option "sf_log_table")
void launch_sf_direct(const int32_t *counts, int64_t n, int S, SelArgs a, FitWork w, unsigned int *hist, uint64_t *lists,
                      int32_t *clear_flag, int cus, int log_table, hipStream_t st);
// region_kernels.hip — offsets, window sums, count join, background, region assembly
void launch_offsets(const double *fullMean, const double *sf_dev, int64_t n, int S, double theta, int mix,
                    double *out, hipStream_t st);
void launch_window_sums(const int32_t *fragN, const double *fragFM, int64_t nfrag, int S, const int64_t *rptr,
                        int64_t n, int32_t *N, double *FM, hipStream_t st);
size_t count_join_scratch_bytes(int64_t nkeys);
void launch_count_join(const int32_t *bait, const int32_t *oe, int64_t nru, const int64_t *keys,
                       const int32_t *vals, int64_t nkeys, int32_t *out, void *scratch, hipStream_t st);
void launch_fragment_background(const int32_t *bait, const int32_t *oe, int64_t nru, int32_t id_min, int32_t nid,
                                const int64_t *midsum, int32_t S, const double *sj, const double *si, const int32_t *tblb,
                                const int32_t *tlb, const double *T, int32_t ntblb, int32_t ntlb, const double *distfun_dev,
                                double *bmean, double *tmean, double *fullmean, hipStream_t st);
size_t count_join_multi_scratch_bytes(int S, const int64_t *nkeys);
void launch_count_join_multi(const int32_t *bait, const int32_t *oe, int64_t nru, int S, const int64_t *const *keys, const int32_t *const *vals,
                             const int64_t *nkeys, int32_t *out, void *scratch, hipStream_t st);
hipError_t launch_region_assemble(const int32_t *bait, const int32_t *oe, int64_t nru, const int64_t *rptr, int64_t n, int S,
                                  const int64_t *const *keys, const int32_t *const *vals, const int64_t *nkeys, int32_t id_min, int32_t nid,
                                  const int64_t *midsum, const double *sj, const double *si, const int32_t *tblb, const int32_t *tlb,
                                  const double *T, int32_t ntblb, int32_t ntlb, const double *distfun_dev, int32_t *N, double *FM,
                                  void *scratch, int force_generic, hipStream_t st);
size_t count_merge_scratch_bytes(int S, const int64_t *nkeys);
hipError_t launch_count_merge(int pass, int S, const int64_t *const *keys, const int32_t *const *vals, const int64_t *nkeys, int64_t cap,
                              int64_t *keys_out, int32_t *vals_out, void *scratch, int64_t **start_out, int64_t *ntile_out, hipStream_t st);
// post_kernels.hip
size_t bh_workspace_bytes(int64_t n);
int launch_bh_adjust(const double *p, int64_t n, double *padj, char *ws, hipStream_t st);
size_t ihw_workspace_bytes();
void launch_ihw_apply(const double *avDist, const double *pvalue, int64_t n, const double *breaks, const double *weights,
                      int ng, int32_t *group, double *weight, double *wp, double *partials, hipStream_t st);
void launch_cooks_filter(const int32_t *counts, int64_t n, int S, int p, const double *maxCooks, const int32_t *argmax,
                         double cutoff, double *pvalue, unsigned long long *nout, hipStream_t st);
size_t if_workspace_bytes(int64_t n);
int run_independent_filtering(const double *d_bm, const double *d_p, int64_t n, double alpha, double *d_padj, char *ws, hipStream_t st,
                              hipStream_t st2, hipEvent_t fork, hipEvent_t join, chicdiff_results_info *info);  // synchronises (three small read-backs)
size_t ct_workspace_bytes(int64_t n);
int launch_count_table(const int32_t *bait, const int32_t *oe, const int32_t *N, int64_t n, const uint8_t *keep, int32_t max_id,
                       int64_t *keys_out, int32_t *vals_out, char *ws, hipStream_t st);
size_t ru_scan_bytes(int64_t n);
int launch_scan_i64(int64_t *d, int64_t n, void *tmp, size_t tmp_bytes, hipStream_t st);
int launch_ru_count(const int32_t *bait, const int32_t *oe, int64_t n, int s, const int32_t *chr_of, int maxfrag,
                    int64_t *region_ptr, int32_t *minOE, int32_t *maxOE, int *bad, void *tmp, size_t tmp_bytes, hipStream_t st,
                    unsigned int *mask_out = nullptr);  // mask_out (n words, may be NULL): per region, which candidates of its window are kept
void launch_ru_fill(const int32_t *bait, const int32_t *oe, int64_t n, int s, const int32_t *chr_of, int maxfrag,
                    const int64_t *region_ptr, int32_t *ru_bait, int32_t *ru_region, int32_t *ru_oe, hipStream_t st,
                    const unsigned int *mask_in = nullptr);  // mask_in: launch_ru_count's masks (NULL: recomputed)
void launch_region_avdist(const int32_t *bait, const int32_t *oe, const int64_t *ptr, int64_t n, int32_t id_min, int32_t nid,
                          const int64_t *midsum, const int32_t *chr, double *avDist, hipStream_t st);
void launch_count_join_inner(const int32_t *bait, const int32_t *oe, int64_t nru, int S, const int64_t *const *keys,
                             const int32_t *const *vals, const int64_t *nkeys, int32_t *out, hipStream_t st);
void launch_pvalues(const double *stat, int64_t n, double *p, hipStream_t st);
// candidate_kernels.hip — getCandidateInteractions (chicdiff.R:2068-2163)
struct CandArgs {
    const int32_t *bait, *minOE, *maxOE;  // region table, caller's row order
    const double *p;
    int64_t n;
    const int32_t *peak_bait, *peak_oe;
    const double *scores;                 // npeaks x ncols, column-major
    int64_t npeaks;
    int32_t ncols, ncond1, merged;
    double score, pvcut, min_delta;
    int32_t method;                       // CHICDIFF_CAND_MIN | CHICDIFF_CAND_HMP: what group_min_p carries
    int64_t pair_capacity;
    int32_t *group_peak;
    int64_t *group_ptr;
    double *group_min_p, *group_delta;
    int32_t *pair_row;
};
// what the host reads back: the two counts, and the smallest offending row of each refusal (all ones = none)
struct CandResult {
    unsigned long long bad_region, bad_peak_key, dup_peak;
    long long ngroups, npairs;
};
size_t cand_workspace_bytes(int64_t n, int64_t npeaks);
int launch_candidates(const CandArgs &a, char *ws, hipStream_t st, const CandResult **res_out);
void launch_landau_selftest(const double *z, int64_t n, double *out, hipStream_t st);  // out[i] = landau_tail(z[i]) (devmath.h)
// control_kernels.hip — the seeded draws of getControlRegionUniverse (chicdiff.R:430-481)
struct CtrlArgs {
    const int32_t *ru_bait;               // RU rows in (regionID, otherEndID) order: baitID
    int64_t nru;
    const int64_t *region_ptr;            // n + 1 CSR offsets into them
    const int32_t *minOE, *maxOE;         // per region
    int64_t n;
    const int32_t *bmap_id, *bmap_chr;    // the baitmap in file order: ID, chromosome code of the map (-1 = not on it)
    int64_t nb;
    const int32_t *chr_min, *chr_max;     // HOST, nchr entries: smallest / largest map ID per chromosome code
    int32_t nchr;
    uint64_t seed;
    int32_t *ctrl_bait, *ctrl_oe;         // n entries each, the first m written
    int32_t *max_contact;                 // nchr entries, 0 = no contact
};
// what the host reads back: the two counts, and the smallest offender of each refusal (all ones = none)
struct CtrlResult {
    unsigned long long n_regions, m, bad_bait, bad_region, cap_k;
};
size_t ctrl_workspace_bytes(int64_t n, int32_t nchr);
int launch_control_draws(const CtrlArgs &a, const int32_t *range_lo, const int32_t *range_hi, const int32_t *range_code, int nranges, char *ws,
                         hipStream_t st, const CtrlResult **res_out);
// chicago_kernels.hip — the Chicago background tables of one replicate (chicdiff.R:656-692, 538-548)
struct ChicagoArgs {
    const int32_t *bait, *oe;                          // one row per observed pair, any order
    const double *s_j, *s_i, *Tmean, *refBinMean;      // NaN = NA
    const int32_t *tblb, *tlb, *distbin;               // level codes, -1 = NA
    int64_t nrows;
    int32_t id_min, nid, ntblb, ntlb, ndistbin;
    double *sj, *si;                                   // nid
    int32_t *tblb_of, *tlb_of;                         // nid
    double *T, *ref;                                   // ntblb x ntlb; ndistbin + 1
};
size_t chicago_workspace_bytes(int32_t nid);
void launch_chicago_tables(const ChicagoArgs &a, int stage, int merge, char *ws, hipStream_t st, const uint32_t **status_out);
// countput_kernels.hip — countput of one condition (chicdiff.R:708-735, 754-768)
struct CountputRep {                                   // one replicate's columns (device pointers) and its first global row
    const int32_t *bait, *oe, *N;
    const double *Bmean, *score, *distSign;
    int64_t offset;
};
struct CountputArgs {
    int32_t nrep;
    const CountputRep *reps;                           // HOST, nrep entries; must stay alive until the stream has been synchronised
    int64_t n;                                         // sum of the replicates' rows, 1 <= n < 2^31
    int32_t id_min, nid;
    const int64_t *midsum;
    const int32_t *chr;
    int32_t *out_bait, *out_oe;                        // n entries each, the first ngroups written
    double *Nav, *Bav, *score, *mid;
};
// what the host reads back
struct CountputResult {
    unsigned long long nkept, ngroups;
};
size_t countput_workspace_bytes(int64_t n);
int launch_countput(const CountputArgs &a, char *ws, hipStream_t st, const CountputResult **res_out);
// chinput_kernels.hip — the body of a .chinput file on the device -> its three int32 columns (chicdiff.R:828, :849).  `text` is 16-byte
// aligned and holds nbytes >= 1 bytes; ws holds chinput_workspace_bytes(nbytes).  _count (mark pass) and _scan leave the row count in
// **nrows_out; _parse then writes the rows below `cap` and takes the minimum offset of the malformed lines into **bad_out (all ones: none)
size_t chinput_workspace_bytes(int64_t nbytes);
int launch_chinput_count(const unsigned char *text, int64_t nbytes, char *ws, hipStream_t st, const int64_t **nrows_out,
                         const unsigned long long **bad_out);
int launch_chinput_scan(int64_t nbytes, char *ws, hipStream_t st);
void launch_chinput_parse(const unsigned char *text, int64_t nbytes, int ib, int io, int in, int32_t *bait, int32_t *oe, int32_t *N, int64_t cap,
                          char *ws, hipStream_t st);
// objective_probe.hip — the dispersion objective on its own (objective_probe_kernel): K points a[i * K + k] per row of a prepared fit
// (w.rowpack: launch_prep), evaluated row per lane (live_rows = 0) or with `live_rows` rows per wave in the samples-across-lanes layout the
// line search would choose for that many; returns the lanes per row of that layout (1: row per lane), or -1 if the search has no
// samples-across-lanes layout for that S and number of rows (nothing is launched then)
struct ObjectiveProbe {
    const double *a;           // n x K evaluation points, log(alpha)
    int K;
    const double *prior_mean;  // per row, or NULL: no prior (the gene-wise search's objective)
    double prior_isig;         // 1 / prior variance
    int live_rows;
    double *lp, *dlp, *alpha;  // n x K
    double *mu;                // S x n: the means the row's evaluations used
};
int launch_objective_probe(FitDims d, FitWork w, Opts o, const ObjectiveProbe &pb, hipStream_t st);
// selftest_kernels.hip — the device math on its own (tests)
void launch_math_selftest(int op, const double *x, int64_t n, double *out, hipStream_t st);
void launch_math3_selftest(int op, const double *x, const double *y, int64_t n, const double *logfact, double *out, double *out2, hipStream_t st);
// table_text_kernels.hip — a table of device columns as text (the rule: include/chicdiff_hip.h, above chicdiff_hip_table_text_dev).
// The descriptors travel as a kernel argument (2 KiB): every lane reads the same one, through the scalar cache.
struct TtCol {
    const void *data;           // device: n values of the column's kind; CHICDIFF_COL_DICT: n int32 codes, or NULL = entry 0 for every row
    const int32_t *dict_off;    // device: ndict + 1 offsets into dict_bytes
    const uint8_t *dict_bytes;  // device
    int32_t kind, ndict;
};
struct TtCols {
    int32_t ncol, sep;
    TtCol col[CHICDIFF_TABLE_MAX_COLUMNS];
};
// what the host reads back after the length pass and the scan
struct TtResult {
    int64_t nbytes;    // bytes of the whole text (written by the scan: the last tile's end)
    int32_t bad_code;  // != 0: a dictionary code >= the number of entries was met (it is written as an empty cell)
    int32_t _pad;
};
size_t table_text_workspace_bytes(int64_t n);
// _len: the length pass, _scan: the scan of the tile totals (n >= 1), enqueued on st; *res_out (inside ws) is valid once st has been
// synchronised after both.
// _write: the write pass; `out` has room for the nbytes the length pass found.
int launch_table_text_len(const TtCols &t, int64_t n, char *ws, hipStream_t st, const TtResult **res_out);
int launch_table_text_scan(int64_t n, char *ws, hipStream_t st);
void launch_table_text_write(const TtCols &t, int64_t n, uint8_t *out, char *ws, hipStream_t st);
void launch_format_double_selftest(const double *x, int64_t n, uint8_t *text, int32_t *len, hipStream_t st);

}  // namespace cd
