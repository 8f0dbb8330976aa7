// disp_objective.h — the dispersion objective of the line searches: a row's record -> LDS (load_row_mu), the log posterior of
// log(alpha) and its derivative row per lane (eval_point) and with the samples spread across lanes (eval_point_spread).
// Included by disp_kernels.hip where this text stood until the objective got a probe of its own
// (objective_probe.hip) — a kernel added to disp_kernels.hip itself changes the code the compiler generates for the search
// kernels there (registers, schedule: tools/device_code_diff.py), a second translation unit does not.
#pragma once
#include "common.h"
#include "devmath.h"

namespace cd {

constexpr int kChunk = 64;   // rows a wave takes from the global queue per atomic (at most: DispArgs::chunk)
constexpr int kTabSlots = 10;  // LDS slots (64 doubles each) of a wave's prefix table = its samples-across-lanes exchange area (128 entries of 36 bytes)
static inline size_t disp_lds_per_wave(int S) { return (size_t)kTabSlots * 64 * 8 + (size_t)S * 64 * 12 + 3 * 64 * 4; }
enum Phase : int { PH_NEED = 0, PH_INIT = 1, PH_SEARCH = 2, PH_DONE = 5 };

// One row of FitWork::rowpack -> the lane's LDS column, with mu_j = max(nf_j * groupmean_g, minmu) formed on the way (what the
// line search needs of nf_j).  All of the record's 16-byte loads are in flight before the first is used (S a multiple of four up
// to 16: one round trip instead of one per four samples), and the all-zero flag comes with the record (sign bit of the first header
// word, set by prep) instead of from a load of its own in front of it.  Returns false for an all-zero row.
__device__ __forceinline__ double max_num(double x, double m) {  // fmax() without the canonicalising copies of its operands
    double r;
    asm("v_max_f64 %0, %1, %2" : "=v"(r) : "v"(x), "v"(m));
    return r;
}
template <int Q>  // S = 4 Q
__device__ __forceinline__ bool load_row_mu_fixed(const char *row, double *s_nf, int *s_y, int lane, uint64_t gmask, double minmu) {
    const double2 *p = reinterpret_cast<const double2 *>(row);
    const int4 *py = reinterpret_cast<const int4 *>(row + kRowHdr + 32 * Q);
    const double2 h0 = p[0];  // the two group means; sign bit of the first: all-zero row
    const int4 prof = *reinterpret_cast<const int4 *>(row + 16);  // the count profile (prep)
    double2 f[2 * Q];
    int4 y[Q];
#pragma unroll
    for (int k = 0; k < 2 * Q; k++) f[k] = p[2 + k];
#pragma unroll
    for (int k = 0; k < Q; k++) y[k] = py[k];
    // (no branch on the flag here: an all-zero row's values go to the lane's LDS column like any other's and are never used —
    // with a branch the compiler moves the loads behind it, i.e. behind the wait for the header.)  The sample's group is a bit
    // of a wave-uniform word; it is taken from a copy the compiler cannot see through, or it builds all S lane masks outside
    // the launch's main loop and spills them.
    uint32_t gbits = (uint32_t)gmask;
    asm volatile("" : "+s"(gbits));
#pragma unroll
    for (int k = 0; k < 2 * Q; k++) {
        s_nf[(2 * k) * 64 + lane] = max_num(f[k].x * (((gbits >> (2 * k)) & 1u) ? h0.y : h0.x), minmu);
        s_nf[(2 * k + 1) * 64 + lane] = max_num(f[k].y * (((gbits >> (2 * k + 1)) & 1u) ? h0.y : h0.x), minmu);
    }
#pragma unroll
    for (int k = 0; k < Q; k++) {
        s_y[(4 * k) * 64 + lane] = y[k].x; s_y[(4 * k + 1) * 64 + lane] = y[k].y;
        s_y[(4 * k + 2) * 64 + lane] = y[k].z; s_y[(4 * k + 3) * 64 + lane] = y[k].w;
    }
    s_y[(4 * Q) * 64 + lane] = prof.x;
    s_y[(4 * Q + 1) * 64 + lane] = prof.y;
    s_y[(4 * Q + 2) * 64 + lane] = prof.z;
    return __double2hiint(h0.x) >= 0;
}
__device__ __forceinline__ bool load_row_mu(const char *row, int S, double *s_nf, int *s_y, int lane, uint64_t gmask, double minmu) {
    if (S == 8) return load_row_mu_fixed<2>(row, s_nf, s_y, lane, gmask, minmu);
    if (S == 4) return load_row_mu_fixed<1>(row, s_nf, s_y, lane, gmask, minmu);
    if (S == 16) return load_row_mu_fixed<4>(row, s_nf, s_y, lane, gmask, minmu);
    if (S == 12) return load_row_mu_fixed<3>(row, s_nf, s_y, lane, gmask, minmu);
    double hdr[2];
    {
        const double2 h0 = reinterpret_cast<const double2 *>(row)[0];
        hdr[0] = h0.x; hdr[1] = h0.y;
    }
    if (__double2hiint(hdr[0]) < 0) return false;
    const double *pf = reinterpret_cast<const double *>(row + kRowHdr);
    const int *py = reinterpret_cast<const int *>(row + kRowHdr + 8 * S);
    const int4 prof = *reinterpret_cast<const int4 *>(row + 16);  // the count profile (prep)
    for (int j = 0; j < S; j++) {
        s_nf[j * 64 + lane] = max_num(pf[j] * (((gmask >> j) & 1) ? hdr[1] : hdr[0]), minmu);
        s_y[j * 64 + lane] = py[j];
    }
    s_y[S * 64 + lane] = prof.x;
    s_y[(S + 1) * 64 + lane] = prof.y;
    s_y[(S + 2) * 64 + lane] = prof.z;
    return true;
}

struct DispArgs {
    const int32_t *counts;
    const double *nf;
    FitDims d;
    FitWork w;
    Opts o;
    unsigned long long *stamps;  // CHICDIFF_DIAG builds only (make DIAG=1): per wave timestamps and tick counts
    int spread;                  // 0 = row-per-lane evaluation only (option "line_search_spread", for the bit-identity test)
    const int32_t *order;        // gene-wise launch: the schedule (order_*); NULL = rows 0..n-1 through the queue (MAP, option "line_search_schedule" 0)
    int deal;                    // entries per group of the static deal (0 = by the number of entries per wave)
    int prefetch;                // 1 = warm the cache lines of the rows handed out next
    int chunk;                   // rows per dequeue (<= kChunk)
    int32_t *gridlist;           // rows whose line search did not converge: fitDispGrid's two stages run in disp_grid_kernel (round 6)
    unsigned int *gridcount;     // ... and their number
    int prio;                    // > 0: a wave raises its issue priority (s_setprio) by one level per `prio` iterations of its oldest search
    unsigned int nfront;         // gene-wise launch with filler waves: the number of front waves (the rest of the grid are fillers); 0 = no fillers
    int filler_stop;             // ... fillers stop claiming at this share (percent) of the front's own chunks
};
// make ISA_MARK=1 (tools/isa_account.py): comment lines in the generated assembly that delimit the parts of a tick; a volatile asm
// statement also keeps the compiler from moving code across it, so the marked build is for counting, not for running
#ifdef CHICDIFF_ISA_MARK
#define MARK(name) asm volatile("; MARK " name)
#else
#define MARK(name)
#endif
#ifdef CHICDIFF_DIAG
#define DIAG(...) __VA_ARGS__
constexpr int kStampSlots = 36;  // start, queue-empty, exit (s_memrealtime), live rows at queue-empty, ticks after queue-empty: row-per-lane / spread / burst, all ticks, s_memtime cycles after queue-empty in row / spread / burst ticks, ..., [34] role (0 front / no roles, 1 filler), [35] where the wave ran (XCC_ID << 16 | HW_ID's low half)
#else
#define DIAG(...)
#endif

// log posterior of a = log(alpha) and its derivative for one row held in LDS (A2.6).
//
// With r = 1/alpha, the per-sample terms of DESeq2's log_posterior / dlog_posterior are
//   lgamma(y+r) - lgamma(r) - y log(mu+r) - r log(1+mu alpha)            (value)
//   digamma(r) - digamma(y+r) + log(1+mu alpha) - mu alpha/(1+mu alpha) + y/(mu+r)   (derivative)
// and are evaluated here as
//   * log(mu+r) = log(1+mu alpha) - a, so one log L covers both logs;
//   * y is an integer count: lgamma(y+r)-lgamma(r) = log prod_{i<n}(r+i) + [lgS(y+r)-lgS(r+n)]
//     with n = min(y, nr), nr = the number of unit steps that lift r to >= 10 (per row and tick),
//     lgS = Stirling's series (valid as both arguments are >= 10); likewise for digamma with the
//     derivative of the product.  Samples with y <= nr need no Stirling term, samples on rows
//     with alpha <= 0.1 need no product;
//     The nr prefix products P_1 .. P_nr are tabulated once per row and tick in LDS (P_0 = 1); the harmonic sums are not: summed
//     over the samples they are sum_{i<nr} c_i / (r+i) with the row's count profile c_i = #{j : y_j > i} (CountProfile above),
//     ten terms at row level (round 6; before: H_n tabulated beside P_n, 22 LDS slots per lane instead of 10);
//   * the products of all samples are multiplied up (mantissa/exponent) and logged ONCE per row.
// mu_j = max(nf_j * groupmean_g, minmu) sits in LDS (formed when the row is staged).
struct RowConsts {  // what depends only on the evaluation point a = log(alpha)
    double a, alpha, r, lgS0, dgS0;
    int nr;
};
__device__ __forceinline__ RowConsts row_consts(double a, const LogEntry *lt, const ExpEntry *et) {
    RowConsts c;
    c.a = a;
    c.alpha = texp(a, et);
    c.r = rcp(c.alpha);
    c.nr = c.r < 10.0 ? (int)ceil(10.0 - c.r) : 0;  // unit steps lifting r to r0 = r + nr >= 10
    const double r0 = c.r + (double)c.nr;
    stirling(r0, tlog(r0, lt), rcp(r0), c.lgS0, c.dgS0);
    return c;
}
struct Acc {  // sums over samples
    double ll = 0, sd = 0, wA = 0, wB = 0, dA = 0, dB = 0;
    double pm = 1.0;  // product of the samples' shift products (mantissas) ...
    int pe = 0;       // ... and of their binary exponents
};
// One sample's contribution as five finished values, and the step that folds them into the row sums.
// The library is compiled with -ffp-contract=off and every fused operation is written out, so the two
// evaluation layouts below (row per lane / samples across lanes) produce the same bits: both call
// sample_values() on the same inputs and both fold the S results in sample order with accumulate().
struct SampleVals {
    double wj, pm, tll, tsd;
    int pe;
};
// P = prod_{i<n}(r+i) for n = min(y, nr) (the harmonic sums H_n of the derivative are added at row level: harmonic_row)
// mu = max(nf_j * groupmean_g, minmu) does not change during a row's search: it is formed once, when the row is staged, and kept in
// the LDS column in place of nf_j (round 3: five instructions per sample and tick less, two shuffled operands less per
// samples-across-lanes tick; same product, same bits)
__device__ __forceinline__ SampleVals sample_values(const RowConsts &c, double mu, int yi, double P, const LogEntry *lt) {
    SampleVals v;
    const double y = (double)yi;
    const double ma = mu * c.alpha;
    const double t = 1.0 + ma;
    const double rt = rcp(t);
    const double L = tlog1p_from(ma, t, rt, lt);
    v.wj = mu * rt;  // 1 / (1/mu + alpha)
    double dlg = 0.0, ddg = 0.0;
    v.pe = __builtin_amdgcn_frexp_exp(P);
    v.pm = __builtin_amdgcn_frexp_mant(P);
    // (Measured, round 4: the two halves of a sample — log1p(mu alpha) with its reciprocal, the Stirling difference at z = y + r
    // with its logarithm and reciprocal — written side by side and branch-free, so that the compiler interleaves the two
    // dependency chains: bit-identical, 207 VGPRs instead of 196, and no faster — gene-wise 1.560 -> 1.565 ms at 2 M x 8,
    // 0.603 -> 0.614 at 250 k.  profiles/r04_ab_line_search_trims.txt)
    if (yi > c.nr) {
        const double z = y + c.r;
        double lgz, dgz;
        stirling(z, tlog(z, lt), rcp(z), lgz, dgz);
        dlg = lgz - c.lgS0;
        ddg = dgz - c.dgS0;
    }
    v.tll = fma(-c.r, L, fma(-y, L - c.a, dlg));          // dlg - y (L - a) - r L
    v.tsd = fma(y * c.alpha, rt, fma(-ma, rt, L - ddg));  // L - ddg - ma/t + y alpha/t
    return v;
}
__device__ __forceinline__ void accumulate(Acc &acc, const SampleVals &v, bool g) {
    // the sample's group is wave-uniform: multiply by an exact 1.0 / 0.0 (scalar operands) instead of selecting
    // registers — x*1 + s and x*0 + s round exactly like s + x and s, at 6 instructions instead of 14
    const double gB = g ? 1.0 : 0.0, gA = g ? 0.0 : 1.0;
    const double tA = v.wj * gA, tB = v.wj * gB;
    acc.wA += tA;
    acc.wB += tB;
    acc.dA = fma(-tA, v.wj, acc.dA);
    acc.dB = fma(-tB, v.wj, acc.dB);
    acc.pe += v.pe;
    acc.pm *= v.pm;
    acc.ll += v.tll;
    acc.sd += v.tsd;
}
// sum over the samples of H_{min(y_j, nr)} = sum_{i < nr} c_i / (r + i), i ascending, from the row's count profile (three ints, ten
// bytes).  TABLE: the same ten steps also leave the prefix products P_1 .. P_10 in the lane's LDS column (entries beyond the lane's nr
// are never read; all ten steps in every lane, no trip count: round 4).  Both evaluation layouts call this with the same operands —
// same bits.  r < 6e30 keeps r^10 finite.
template <bool TABLE>
__device__ __forceinline__ double harmonic_row(const RowConsts &c, unsigned int w0, unsigned int w1, unsigned int w2, double *s_tab, int lane) {
    // bytes i >= nr of the profile do not count
    const unsigned int nr = (unsigned int)c.nr;
    const unsigned int a = nr < 4u ? nr : 4u, b = nr < 4u ? 0u : (nr < 8u ? nr - 4u : 4u), d = nr < 8u ? 0u : nr - 8u;
    w0 &= a == 4u ? 0xffffffffu : ((1u << (8u * a)) - 1u);
    w1 &= b == 4u ? 0xffffffffu : ((1u << (8u * b)) - 1u);
    w2 &= (1u << (8u * d)) - 1u;
    // The sum is carried as a numerator over the prefix product, N_{i+1} = N_i (r + i) + c_i P_i with H = N_10 / P_10 (the P / Q
    // recurrence of lgamma_digamma(), devmath.h): one reciprocal per tick instead of one per step (round 22: ten v_rcp_f64 with two
    // Newton steps each were 9 % of a bulk tick's issue cycles).  P's own operations and their order are those of the table, so the
    // table keeps its bits; a lane whose profile is masked to zero (nr = 0) has N = 0 and H = 0 as long as P is finite — 0 x inf would be
    // NaN where the former sum of c_i / (r + i) was an exact 0.  P_10 < r^10 (1 + 9 / r)^10 is finite for r below ~ 1e30, and every caller
    // keeps a = log(alpha) inside [-30, 10] (the searches clamp their steps to it, the grid starts at log(1e-8)): r <= e^30 ~ 1.1e13.
    double P = 1.0, N = 0.0, zz = c.r;
#ifdef HR_ROLLED
#pragma unroll 1
#else
#pragma unroll
#endif
    for (int i = 0; i < 10; i++) {
        const unsigned int w = i < 4 ? w0 : (i < 8 ? w1 : w2);
        const double ci = (double)((w >> (8 * (i & 3))) & 0xffu);
        N = fma(N, zz, ci * P);
        P *= zz;
        if (TABLE) s_tab[i * 64 + lane] = P;
        zz += 1.0;
#ifdef HR_SCHED_BARRIER
        __builtin_amdgcn_sched_barrier(0);
#endif
    }
    return N * rcp(P);
}
__device__ __forceinline__ void finish_point(const Acc &acc, const RowConsts &c, double Hrow, bool p2, bool use_prior,
                                             double prior_mean, double prior_isig, double &lp, double &dlp,
                                             const LogEntry *lt) {
    const double ll = acc.ll + fma((double)acc.pe, 0.69314718055994530942, tlog(acc.pm, lt));
    double cr, dcr;
    if (p2) {
        cr = -0.5 * tlog(acc.wA * acc.wB, lt);
        dcr = -0.5 * (acc.dA * rcp(acc.wA) + acc.dB * rcp(acc.wB));
    } else {
        cr = -0.5 * tlog(acc.wA, lt);
        dcr = -0.5 * (acc.dA * rcp(acc.wA));
    }
    double pr = 0, dpr = 0;
    if (use_prior) {
        const double dd = c.a - prior_mean;
        pr = -0.5 * dd * dd * prior_isig;
        dpr = -dd * prior_isig;
    }
    lp = ll + pr + cr;
    dlp = (c.r * c.r * (acc.sd - Hrow) + dcr) * c.alpha + dpr;
}

// Row-per-lane evaluation: all S samples of the row in LDS column `slot` (the lane's own row; in disp_grid_kernel the column of
// the row whose grid point the lane evaluates), the prefix table in the lane's own column.
__device__ __forceinline__ void eval_point(const double *s_nf, const int *s_y, double *s_tab, int lane, int slot, int S, uint64_t gmask,
                                           bool p2, double a,
                                           bool use_prior, double prior_mean, double prior_isig,
                                           double &lp, double &dlp, double &alpha_out, const LogEntry *lt, const ExpEntry *et
                                           DIAG(, unsigned long long *tm)) {
    MARK("row:begin");
    DIAG(tm[0] = __builtin_amdgcn_s_memtime();)
    const RowConsts c = row_consts(a, lt, et);
    alpha_out = c.alpha;
    MARK("row:row_consts_end");
    DIAG(tm[1] = __builtin_amdgcn_s_memtime();)
    // per-tick table (LDS, [entry][lane]): P_n for n = 1..10, and the row-level harmonic sum from the count profile of the row in
    // column `slot` (harmonic_row: ten unconditional steps — in-kernel timers, round 4: a loop to the lane's own nr ran, in SIMD, to the
    // wave's largest, and unrolled by eight plus a remainder loop)
    double Hrow = 0.0;
    if (__ballot(c.nr > 0) != 0ull)
        Hrow = harmonic_row<true>(c, (unsigned int)s_y[S * 64 + slot], (unsigned int)s_y[(S + 1) * 64 + slot], (unsigned int)s_y[(S + 2) * 64 + slot], s_tab, lane);
    MARK("row:table_end");
    DIAG(tm[2] = __builtin_amdgcn_s_memtime();)
    Acc acc;
    for (int j = 0; j < S; j++) {
        const int yi = s_y[j * 64 + slot];
        const int n = yi < c.nr ? yi : c.nr;
        const bool g = (gmask >> j) & 1;
        const double Pt = s_tab[((n > 0 ? n : 1) - 1) * 64 + lane];  // (n = 0: P_0 = 1; the entry read instead is never used)
        accumulate(acc, sample_values(c, s_nf[j * 64 + slot], yi, n > 0 ? Pt : 1.0, lt), g);
    }
    MARK("row:samples_end");
    DIAG(tm[3] = __builtin_amdgcn_s_memtime();)
    finish_point(acc, c, Hrow, p2, use_prior, prior_mean, prior_isig, lp, dlp, lt);
    MARK("row:finish_end");
    DIAG(tm[4] = __builtin_amdgcn_s_memtime();)
}

// Samples-across-lanes evaluation for the end of the launch.  Once the queue is empty every wave is left
// with a dozen rows that still need up to ~130 serial evaluations (flat likelihoods: DESeq2's step size
// decays faster than the search converges, then the grid takes over), and a row-per-lane tick costs the same
// ~1600 instructions whether 64 lanes or one are busy.  When at most 64/G rows are live (G = 2^lg lanes per row), the
// g-th live row is evaluated by lanes G*g .. G*g+G-1 — one sample each when G >= S, else samples jj, jj + G, ... (S = 8:
// four lanes per row for 9-16 live rows, two for 17-32; round 3) —: every lane rebuilds the row
// constants (same instructions, no extra cost in SIMD), walks its own prefix product, computes its sample's
// five values, then every lane of the group folds the S results in sample order (so each holds the row's
// sums) and the owning lane picks the result up.  Same functions, same operand values, same order of the
// floating-point operations as eval_point(): the bits do not depend on which layout evaluated a tick,
// hence not on the schedule (tests/test_gpu_parity.py::test_line_search_layouts_agree_bit_for_bit).
// Gain at 2 M rows: 1 % of the gene-wise launch at S = 8, 4 % at S = 4, 10 % at S = 16.
// (Measured and dropped: handing the stragglers to a second, densely packed launch — a wave's tick takes
// ~5 us alone or with a neighbour on its SIMD, the tail is bound by the ~130 serial ticks, not by issue.)
// Which lanes evaluate which live row in a samples-across-lanes tick.  It depends only on the set of live lanes (and, for the MAP
// search, on the rows' prior means), so the launch's end — tick after tick with the same few rows — builds it once per change of
// that set (round 5) instead of once per tick.
struct SpreadMap {
    unsigned long long mask;  // the live lanes it was built for
    int lg;                   // log2(lanes per row); -1: the rows do not fit (row-per-lane tick)
    int owner;                // the lane whose LDS column holds this lane's row
    int src;                  // first lane of the group that evaluates this lane's own row (live lanes)
    bool has;                 // this lane's group has a row
    double pm_o;              // the row's prior mean (MAP)
};
__device__ __forceinline__ SpreadMap spread_map(double *s_x, int lane, int lg, unsigned long long actmask, bool active, bool use_prior, double prior_mean) {
    SpreadMap m;
    m.mask = actmask;
    m.lg = lg;
    const int grp = lane >> lg;
    // owner of group g = the g-th live lane: every live lane leaves its number at its rank among the live lanes, group g reads entry
    // g (one LDS round trip instead of a walk over the set bits: ~50 instructions per tick of a launch's latency-bound end)
    const int nact = __popcll(actmask);
    const int myrank = (int)__builtin_amdgcn_mbcnt_hi((uint32_t)(actmask >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)actmask, 0u));
    int *s_own = reinterpret_cast<int *>(s_x);  // in the exchange area itself: read here, before an evaluation writes the area again (a wave's LDS operations execute in order)
    __builtin_amdgcn_wave_barrier();            // (every lane has read the last evaluation's values)
    if (active) s_own[myrank] = lane;
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
    m.has = grp < nact;
    m.owner = m.has ? s_own[grp] : 0;
    __builtin_amdgcn_wave_barrier();            // (... and the look-up is over before the area is written again)
    m.src = (active ? myrank : 0) << lg;  // an active lane's group is its rank among the active lanes
    m.pm_o = use_prior ? __shfl(prior_mean, m.owner) : 0.0;
    return m;
}
__device__ __forceinline__ void eval_point_spread(const double *s_nf, const int *s_y, double *s_x, int lane, int S, const SpreadMap &map, uint64_t gmask,
                                                  bool p2, double a_eval,
                                                  bool use_prior, double prior_isig,
                                                  double &lp, double &dlp, double &alpha_out, const LogEntry *lt, const ExpEntry *et
                                                  DIAG(, unsigned long long *tm)) {
    DIAG(tm[0] = __builtin_amdgcn_s_memtime();)
    // lanes per row L = 2^lg: one sample per lane when L >= S (at most 64 / L rows), else samples jj, jj + L, ... per lane — the
    // layout also serves 9 .. 32 live rows (S = 8: four or two lanes per row), where a row-per-lane tick would still walk all S
    // samples in every lane
    const int lg = map.lg;
    const int L = 1 << lg, grp = lane >> lg, jj = lane & (L - 1), R = 64 >> lg;
    const bool has = map.has;
    const int owner = map.owner;
    MARK("spread:owner_walk_end");
    DIAG(tm[1] = __builtin_amdgcn_s_memtime();)
    const double a_o = __shfl(a_eval, owner);
    const double pm_o = map.pm_o;
    const RowConsts c = row_consts(a_o, lt, et);
    MARK("spread:row_consts_end");
    DIAG(tm[2] = __builtin_amdgcn_s_memtime();)
    // the five values of every sample pass through the wave's prefix-table area (idle in this layout), [value][sample R + group]:
    // each lane then reads its group's samples — four samples' loads in flight at a time, same address within a group (a
    // broadcast), neighbouring banks across groups — and folds them in sample order.  (Round 2 fetched them with nine
    // ds_bpermute per sample inside the fold loop: one LDS round trip per sample on the critical path of a tick that is all
    // latency.)  The area holds 128 entries (4 x 128 doubles + 128 ints of the 10 x 64 doubles: round 6, when the table lost its
    // harmonic half); a layout of S R <= 256 entries goes through it in two rounds of ceil(S / 2) samples each, folded in sample
    // order as before: same bits.
    // the row-level harmonic sum from the owner's count profile (every lane of the group: same instructions, no extra cost in SIMD);
    // skipped — profile reads included — when no row of the wave has r < 10 (the flat-likelihood rows of a launch's end never have)
    double Hrow = 0.0;
    if (__ballot(c.nr > 0) != 0ull) {
        const unsigned int w0 = has ? (unsigned int)s_y[S * 64 + owner] : 0u, w1 = has ? (unsigned int)s_y[(S + 1) * 64 + owner] : 0u;
        const unsigned int w2 = has ? (unsigned int)s_y[(S + 2) * 64 + owner] : 0u;
        Hrow = harmonic_row<false>(c, w0, w1, w2, nullptr, lane);
    }
    int *s_xe = reinterpret_cast<int *>(s_x + 4 * 128);
    Acc acc;
    // one round of the exchange: the samples [j0, j1) of every group's row
    auto round = [&](const int j0, const int j1, const int js) {
        for (int j = js; j < j1; j += L) {  // (the same trip count in every lane of a group up to the guard)
            const int yi = has ? s_y[j * 64 + owner] : 0;
            const double nfj = has ? s_nf[j * 64 + owner] : 1.0;
            double P = 1.0;
            {
                const int n = yi < c.nr ? yi : c.nr;
                double zz = c.r;
                for (int i = 0; i < n; i++) {  // the same recurrence as the table of eval_point(), stopped at entry n
                    P *= zz;
                    zz += 1.0;
                }
            }
            MARK("spread:prefix_walk_end");
            const SampleVals v = sample_values(c, nfj, yi, P, lt);
            MARK("spread:sample_end");
            const int e = (j - j0) * R + grp;
            s_x[e] = v.wj;
            s_x[128 + e] = v.pm;
            s_x[256 + e] = v.tll;
            s_x[384 + e] = v.tsd;
            s_xe[e] = v.pe;
        }
        MARK("spread:exchange_store_end");
        DIAG(if (j0 == 0) tm[3] = __builtin_amdgcn_s_memtime();)
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
        __builtin_amdgcn_wave_barrier();
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
        for (int q0 = j0; q0 < j1; q0 += 4) {
            SampleVals u[4];
#pragma unroll
            for (int t = 0; t < 4; t++) {
                const int src = ((q0 + t < j1 ? q0 + t : q0) - j0) * R + grp;
                u[t].wj = s_x[src];
                u[t].pm = s_x[128 + src];
                u[t].tll = s_x[256 + src];
                u[t].tsd = s_x[384 + src];
                u[t].pe = s_xe[src];
            }
#pragma unroll
            for (int t = 0; t < 4; t++)
                if (q0 + t < j1) accumulate(acc, u[t], (gmask >> (q0 + t)) & 1);
        }
        __builtin_amdgcn_wave_barrier();  // (the area is written again only after every lane has read it)
    };
    if (S * R <= 128) {  // (the usual case at a launch's end: one round, as before round 6)
        round(0, S, jj);
    } else {
        const int Sh = (S + 1) >> 1;
        round(0, Sh, jj);
        round(Sh, S, jj >= Sh ? jj : jj + (((Sh - jj + L - 1) >> lg) << lg));  // (this lane's first sample of the second round)
    }
    MARK("spread:fold_end");
    DIAG(tm[4] = __builtin_amdgcn_s_memtime();)
    double lp_g, dlp_g;
    finish_point(acc, c, Hrow, p2, use_prior, pm_o, prior_isig, lp_g, dlp_g, lt);
    MARK("spread:finish_end");
    DIAG(tm[5] = __builtin_amdgcn_s_memtime();)
    const int src = map.src;
    lp = __shfl(lp_g, src);
    dlp = __shfl(dlp_g, src);
    alpha_out = __shfl(c.alpha, src);
    MARK("spread:pickup_end");
    DIAG(tm[6] = __builtin_amdgcn_s_memtime();)
}

}  // namespace cd
