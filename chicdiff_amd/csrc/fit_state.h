// fit_state.h — the fit's global state machines, shared between device and host.
//
// Everything global in one fit is a SUM over rows followed by a small scalar
// decision: Gamma-GLM trend IRLS (DESeq2 parametricDispersionFit + glm.fit, Appendix A3), exact
// medians by radix select (size factors A1, MAD A3), prior variance (A4).  The decisions live
// here as plain inline functions over `FitScalars`, so that
//   * the GPU runs them in one-thread kernels (no host round trip per IRLS step), and
//   * the row-sharded path (sum-all-reduce between the per-rank partial sums and the decision)
//     can be exercised on CPU, world_size 2 over gloo, with exactly this code
//     (tests/harness/shard_harness.cpp).
// No HIP types here: compiles with hipcc and with g++.
#pragma once
#include <math.h>
#include <stdint.h>

#if defined(__HIPCC__)
#define CD_HD __host__ __device__ inline
#else
#define CD_HD inline
#endif

namespace cd {

constexpr int kMaxS = 64;          // samples per fit (group mask is one 64-bit word)
constexpr int kSelBits = 12;       // radix-select digit width
constexpr int kSelBins = 1 << kSelBits;
constexpr int kTrendSums = 8;      // dev, sw, swx, swxx, swy, swxy, count, invalid

// Device-resident scalars of one fit; the host reads the struct back once, at the end.
struct FitScalars {
    double colsum[kMaxS];  // column sums of nf over non-all-zero rows (then all-reduced)
    double nnz;            // number of non-all-zero rows (double: goes through the f64 all-reduce)
    double xim;            // mean_j 1/colMeans(nf)_j                  (DESeq2 momentsDispEstimate)
    // trend state machine (parametricDispersionFit + glm.fit)
    double coefs[2];       // outer-loop coefficients (define the `good` set)
    double b[2];           // inner IRLS iterate
    double devold;
    int32_t inner_it, outer_it, phase, finished, failed, conv, neg_counts /* a count < 0 (NA_integer_) was seen by prep */,
        trend_local /* dispFit[] holds the local-regression trend (DESeq2 fitType "local"): coefs are not used */;
    double nfit;
    // MAD / prior
    double med, mad, varLogDispEsts, dispPriorVar;
    double nres;
    double sumDeviance;
    double nonconv;
    // radix-select state: up to kMaxS columns x 2 ranks (lower / upper median)
    uint64_t sel_prefix[kMaxS * 2];
    double sel_rank[kMaxS * 2];  // remaining 0-based rank inside the current prefix
    double sel_count[kMaxS];     // population per column
    double sel_value[kMaxS * 2]; // selected order statistics
    uint32_t sel_cnt[kMaxS * 2]; // single-rank shortcut: candidates left after two rounds, per (column, slot)
    int32_t sel_fast_done; // 1 = the shortcut resolved every order statistic of the running select
    int32_t spec_next;     // trend: the next pass speculates (trend_step_spec; used by the persistent kernel's own copy of the state only)
    // schedule of the gene-wise line search (disp_kernels.hip: order_*): rows of order[0, ord_na) are dealt out statically,
    // rows of order[ord_na, ord_n) through the queue; all-zero rows are in neither
    int64_t ord_na, ord_n;
    // sharded selects run optimistically (no host look at sel_fast_done): a candidate list that did not fit (massive ties)
    // leaves this set, the host sees it with the fit's final scalars and refits with every histogram round
    int32_t sel_overflow;
    int32_t ord_nb;  // gene-wise schedule: order[ord_nb, ord_n) are the rows that cannot be long (score >= 3.16 and what is behind them): the filler waves' end of the queue
    // what the host reads when a fit ends, gathered here by the fit's last kernel so that ONE copy brings everything back:
    // [0] deviance sum, [1] non-converged rows, [2] all-zero rows, then four verdicts of this rank (all seven summed over the ranks
    // of a sharded fit): [3] trend kernel's grid barrier timed out, [4] negative / NA count, [5] a select's candidate list overflowed
    // in this fit, [6] ... in the size-factor select the caller ran before it; and the size factors of that select
    double final_sums[8];
    double final_sf[kMaxS];
};

// order-preserving map double -> uint64 (NaN never passed in)
CD_HD uint64_t key_of(double x) {
    union { double d; uint64_t u; } c;
    c.d = x;
    return (c.u & 0x8000000000000000ull) ? ~c.u : (c.u | 0x8000000000000000ull);
}
CD_HD double value_of(uint64_t k) {
    union { double d; uint64_t u; } c;
    c.u = (k & 0x8000000000000000ull) ? (k & 0x7fffffffffffffffull) : ~k;
    return c.d;
}

// ---- trend ---------------------------------------------------------------------------------
enum { TR_INNER_START = 0, TR_INNER_ITER = 1 };

CD_HD void trend_init(FitScalars *sc) {
    sc->coefs[0] = 0.1;  // parametricDispersionFit: coefs <- c(.1, 1)
    sc->coefs[1] = 1.0;
    sc->b[0] = 0.1;
    sc->b[1] = 1.0;
    sc->devold = 0;
    sc->inner_it = 0;
    sc->outer_it = 0;
    sc->phase = TR_INNER_START;
    sc->finished = 0;
    sc->failed = 0;
    sc->conv = 0;
    sc->spec_next = 0;
}

// One row's contribution to the fused pass: is it in the `good` set that the coefficients (c0, c1) define, and if so its
// deviance at the iterate (b0, b1) and the weighted-LS sums for the next iterate.
CD_HD void trend_row_at(double c0, double c1, double b0, double b1, double baseMean, double disp, double *v /*[kTrendSums]*/) {
    const double r = disp / (c0 + c1 / baseMean);
    if (!(r > 1e-4 && r < 15)) return;
    const double x = 1.0 / baseMean;
    const double mu = b0 + b1 * x;
    if (!(mu > 0) || !isfinite(mu)) {
        v[7] += 1;
        return;
    }
    v[0] += -2.0 * (log(disp / mu) - (disp - mu) / mu);  // Gamma deviance residual
    const double wt = 1.0 / (mu * mu);                   // glm.fit weight for Gamma/identity
    v[1] += wt;
    v[2] += wt * x;
    v[3] += wt * x * x;
    v[4] += wt * disp;
    v[5] += wt * x * disp;
    v[6] += 1;
}
CD_HD void trend_row(const FitScalars *sc, double baseMean, double disp, double *v /*[kTrendSums]*/) {
    trend_row_at(sc->coefs[0], sc->coefs[1], sc->b[0], sc->b[1], baseMean, disp, v);
}
// A row of a SPECULATIVE pass (trend_step_spec below): besides v, the sums u that the start pass of the NEXT glm() call would
// form if this pass turns out to be the converging one — then coefs := b, so that pass selects with b and evaluates at b.
CD_HD void trend_row_spec(const FitScalars *sc, double baseMean, double disp, double *v, double *u /*[kTrendSums] each*/) {
    trend_row_at(sc->coefs[0], sc->coefs[1], sc->b[0], sc->b[1], baseMean, disp, v);
    trend_row_at(sc->b[0], sc->b[1], sc->b[0], sc->b[1], baseMean, disp, u);
}

// Consume the (all-reduced) sums of one pass: R's glm.fit bookkeeping (epsilon 1e-8, maxit 25)
// inside parametricDispersionFit's outer loop (<= 10 re-selections, stop on sum(log(c/c_old)^2) < 1e-6).
// Returns true when the pass ended a glm() call and the outer loop goes on: the next pass is the start pass of the next call.
// *rel (optional): relative deviance change of an inner pass that did not converge (else left alone).
CD_HD bool trend_consume(FitScalars *sc, const double *s /*[kTrendSums]*/, double *rel) {
    if (sc->finished) return false;
    const double dev = s[0], sw = s[1], swx = s[2], swxx = s[3], swy = s[4], swxy = s[5], cnt = s[6], bad = s[7];
    bool inner_done = false, conv = false;
    if (bad > 0 || cnt < 2) {  // invalid mu (R would step-halve; DESeq2 ends in "fit failed") or no data
        sc->failed = 1;
        sc->finished = 1;
        return false;
    }
    if (sc->phase == TR_INNER_START) {
        sc->devold = dev;
        sc->inner_it = 0;
        sc->phase = TR_INNER_ITER;
    } else {
        const double change = fabs(dev - sc->devold) / (fabs(dev) + 0.1);
        if (change < 1e-8) {
            inner_done = true;
            conv = true;
        } else {
            sc->devold = dev;
            if (rel) *rel = change;
            if (sc->inner_it >= 25) inner_done = true;  // glm.fit maxit, not converged
        }
    }
    if (!inner_done) {
        const double det = sw * swxx - swx * swx;
        const double nb0 = (swxx * swy - swx * swxy) / det, nb1 = (sw * swxy - swx * swy) / det;
        if (!isfinite(nb0) || !isfinite(nb1)) {
            sc->failed = 1;
            sc->finished = 1;
            return false;
        }
        sc->b[0] = nb0;
        sc->b[1] = nb1;
        sc->inner_it++;
        return false;
    }
    const double o0 = sc->coefs[0], o1 = sc->coefs[1];
    sc->coefs[0] = sc->b[0];
    sc->coefs[1] = sc->b[1];
    if (!(sc->coefs[0] > 0 && sc->coefs[1] > 0)) {  // "parametric dispersion fit failed"
        sc->failed = 1;
        sc->finished = 1;
        return false;
    }
    const double l0 = log(sc->coefs[0] / o0), l1 = log(sc->coefs[1] / o1);
    if ((l0 * l0 + l1 * l1 < 1e-6) && conv) {
        sc->finished = 1;
        sc->conv = 1;
        return false;
    }
    sc->outer_it++;
    if (sc->outer_it > 10) {  // "dispersion fit did not converge"
        sc->failed = 2;
        sc->finished = 1;
        return false;
    }
    sc->phase = TR_INNER_START;  // next glm() call: new `good` set, start = coefs
    return true;
}
CD_HD void trend_step(FitScalars *sc, const double *s /*[kTrendSums]*/) { trend_consume(sc, s, nullptr); }

// The same step for a caller whose passes can SPECULATE (the persistent kernel): a pass that was announced as speculative
// (sc->spec_next set by the step before it) brings a second set of sums u, those of trend_row_spec — what the start pass of the
// next glm() call would sum if this pass converges.  If it does and the outer loop goes on, u is consumed here exactly as that
// start pass would be (the bad / cnt check, devold, the new b, inner_it = 1) and the start pass is never run; otherwise u is
// dropped: a wrong prediction costs time only, and coefs, outer_it, conv, failed come out as from trend_step.  u == NULL: the pass
// did not speculate.  Then the step says whether the next pass should: a pure function of the state, so every workgroup of the
// kernel, each running its own copy of the machine, decides the same.  Deviance changes shrink about a hundredfold per inner pass
// (linear convergence), so a change under 1e-5 announces one under 1e-8; and a glm() call after the first starts next to its
// solution, so its first inner pass may already be the last.  Returns true if u was consumed (a pass saved).
CD_HD bool trend_step_spec(FitScalars *sc, const double *s, const double *u /*[kTrendSums] or NULL*/, bool speculate) {
    double rel = 1.0;
    bool used = false;
    if (trend_consume(sc, s, &rel) && u) {
        trend_consume(sc, u, nullptr);
        used = true;
        rel = 1.0;
    }
    sc->spec_next = (speculate && !sc->finished && sc->phase == TR_INNER_ITER && ((sc->outer_it > 0 && sc->inner_it == 1) || rel < 1e-5)) ? 1 : 0;
    return used;
}

// ---- exchange of a pass's partial sums between the workgroups of the persistent trend kernel (option "trend_exchange") ----
// A double travels as two 64-bit words that each say which pass they belong to: (tag << 32) | low half, (tag << 32) | high half,
// tag = pass + 1.  A 64-bit store lands whole, so a word whose tag is the reader's is that pass's half, whatever else has or has
// not landed yet — validity travels inside the data and no fence or counter has to order the two.  Tag 0 is never written: it is
// what the fill at the head of a fit leaves, and no pass accepts it.
CD_HD void xchg_pack(double x, uint32_t tag, uint64_t *lo, uint64_t *hi) {
    union { double d; uint64_t u; } c;
    c.d = x;
    *lo = ((uint64_t)tag << 32) | (c.u & 0xffffffffull);
    *hi = ((uint64_t)tag << 32) | (c.u >> 32);
}
CD_HD bool xchg_accept(uint64_t word, uint32_t tag) { return tag != 0u && (uint32_t)(word >> 32) == tag; }
CD_HD double xchg_unpack(uint64_t lo, uint64_t hi) {
    union { double d; uint64_t u; } c;
    c.u = (hi << 32) | (lo & 0xffffffffull);
    return c.d;
}

// ---- radix select ----------------------------------------------------------------------------
// ranks of the two middle order statistics (R median(): mean of the two for even counts)
CD_HD void sel_begin(FitScalars *sc, int col, double population) {
    sc->sel_count[col] = population;
    const int64_t mi = (int64_t)population;
    sc->sel_rank[2 * col] = (double)((mi - 1) / 2);
    sc->sel_rank[2 * col + 1] = (double)(mi / 2);
    sc->sel_prefix[2 * col] = 0;
    sc->sel_prefix[2 * col + 1] = 0;
}
// does `key` fall under prefix `p` on the bits above `hi`?
CD_HD bool sel_match(uint64_t key, uint64_t p, int hi) { return hi >= 64 || (key >> hi) == (p >> hi); }

// given the (all-reduced) digit histogram `g[0..nb)` for one slot, extend its prefix
CD_HD void sel_pick(FitScalars *sc, int col, int slot, const double *g, int nb, int shift, uint64_t prefix) {
    const double rank = sc->sel_rank[2 * col + slot];
    double cum = 0;
    int b = 0;
    for (; b < nb - 1; b++) {
        if (cum + g[b] > rank) break;
        cum += g[b];
    }
    sc->sel_prefix[2 * col + slot] = prefix | ((uint64_t)b << shift);
    sc->sel_rank[2 * col + slot] = rank - cum;
}
CD_HD double sel_median(const FitScalars *sc, int col) {
    const double lo = value_of(sc->sel_prefix[2 * col]), hi = value_of(sc->sel_prefix[2 * col + 1]);
    return (sc->sel_count[col] > 0) ? (lo + hi) / 2.0 : NAN;
}
static const int kSelShifts[6] = {52, 40, 28, 16, 4, 0};  // 5 x 12 bits + 4 bits
CD_HD bool sel_first_round(int shift) { return shift == 52; }
CD_HD int sel_bits(int shift) { return shift == 0 ? 4 : kSelBits; }

// ---- value-binned select (the MAD step of the persistent trend kernel) ------------------------------------------------------
// The log residuals are well spread (the fullest 1/1024-wide bin holds under 0.1 % of them), so ONE histogram over their values
// — filled by the pass that forms them — finds the bin of the median, and, once the median is known, brackets the median of the
// absolute deviations as well.  The bin function is monotone, so values outside the range land in the end bins and stay exact;
// nothing exact rests on the bracket: the rows below it are counted by comparing |x - med| itself, and a failed check (or a
// list that does not fit) sends the select to the radix rounds above.
constexpr int kVbBins = 15360;     // bins of width 1/1024 over [-7.5, 7.5): 61 440 B of LDS, 15 per thread of the kernel
constexpr double kVbOffset = 7.5, kVbScale = 1024.0;
constexpr int kVbCap = 8000;       // keys per candidate list: what the kernel's freed 64 000 B cache holds
constexpr int kVbSub = 4096;       // second-level bins when a list is narrowed down inside a workgroup
CD_HD int vb_clamp(double t, int nb) {  // t = floor(...): -> [0, nb), NaN and everything below 1 -> 0
    if (!(t > 0)) return 0;
    if (t >= (double)(nb - 1)) return nb - 1;
    return (int)t;
}
CD_HD int vb_bin(double x) { return vb_clamp(floor((x + kVbOffset) * kVbScale), kVbBins); }
CD_HD int vb_sub(double v, double vlo, double scale) { return vb_clamp(floor((v - vlo) * scale), kVbSub); }  // monotone in v for scale >= 0
// over an inclusive cumulative histogram cum[0..nb): the first bin with cum[b] > rank (the last bin if there is none) ...
CD_HD int cum_locate(const uint32_t *cum, int nb, uint32_t rank) {
    int lo = 0, hi = nb - 1;
    while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (cum[mid] > rank) hi = mid;
        else lo = mid + 1;
    }
    return lo;
}
// ... and the entries of bins [b0, b1] (none if b0 > b1)
CD_HD uint32_t cum_range(const uint32_t *cum, int b0, int b1) { return b0 > b1 ? 0u : cum[b1] - (b0 > 0 ? cum[b0 - 1] : 0u); }
// the two middle ranks (R median()) and the bins that hold them; the candidates are the `count` entries of bins binA and binB
// (no entry lies between two neighbouring ranks), `below` entries come before them: the ranks inside the list are rank - below
struct VbPick { uint32_t pop, rankA, rankB, below, count; int binA, binB; };
CD_HD VbPick vb_pick(const uint32_t *cum, int nb) {
    VbPick p = {cum[nb - 1], 0u, 0u, 0u, 0u, 0, 0};
    if (p.pop == 0) return p;
    p.rankA = (p.pop - 1) / 2;
    p.rankB = p.pop / 2;
    p.binA = cum_locate(cum, nb, p.rankA);
    p.binB = cum_locate(cum, nb, p.rankB);
    p.below = cum_range(cum, 0, p.binA - 1);
    p.count = cum_range(cum, p.binA, p.binB);
    return p;
}
// Bounds of #{ |x - med| < rho } from the value histogram: every such x lies in the bins from that of med - rho to that of
// med + rho, and every x in a bin strictly between those two (never an end bin, which holds the values out of range) is one.
CD_HD uint32_t vb_upper(const uint32_t *cum, double med, double rho) { return cum_range(cum, vb_bin(med - rho), vb_bin(med + rho)); }
CD_HD uint32_t vb_lower(const uint32_t *cum, double med, double rho) { return cum_range(cum, vb_bin(med - rho) + 1, vb_bin(med + rho) - 1); }
// Bracket [lo, hi) of the two middle order statistics of |x - med|, on a grid of a quarter bin: lo the largest rho with at most
// rankA values certainly below it (0 always qualifies), hi the smallest with more than rankB (+inf if there is none — then the
// candidates will not fit, except in a tiny fit).  Both conditions are monotone in rho.
CD_HD void vb_bracket(const uint32_t *cum, double med, uint32_t rankA, uint32_t rankB, double *lo, double *hi) {
    const int T = 8 * kVbBins;  // rho up to 30, twice the range
    const double step = 1.0 / (4.0 * kVbScale);
    int a = 0, b = T;
    while (a < b) {
        const int mid = (a + b + 1) >> 1;
        if (vb_upper(cum, med, mid * step) <= rankA) a = mid;
        else b = mid - 1;
    }
    *lo = a * step;
    a = 0;
    b = T + 1;
    while (a < b) {
        const int mid = (a + b) >> 1;
        if (vb_lower(cum, med, mid * step) > rankB) b = mid;
        else a = mid + 1;
    }
    *hi = a > T ? INFINITY : a * step;
}
// After the gather pass has counted, by comparing |x - med| itself, the population, the values below lo and the candidates in
// [lo, hi): do the middle ranks lie inside the list, and does the list fit?  kA, kB: their ranks inside the list.
CD_HD bool vb_check(uint32_t pop, uint32_t below, uint32_t cand, uint32_t cap, uint32_t *kA, uint32_t *kB) {
    if (pop == 0) return false;
    const uint32_t rA = (pop - 1) / 2, rB = pop / 2;
    if (!(below <= rA && rB - below < cand && cand <= cap)) return false;
    *kA = rA - below;
    *kB = rB - below;
    return true;
}

// ---- gathering the candidates after two rounds (sharded shortcut) ------------------------------------
// After two 12-bit rounds only the keys sharing 24 bits with a median are left — a few hundred among millions.
// Sharded, every rank knows how many of them it holds (its own round-2 histogram at the chosen digit), so
// instead of four more histogram rounds: one all-reduce of the per-rank counts (each rank fills its own row),
// every rank writes its candidates at its offset into a zeroed buffer, one all-reduce (a sum of disjoint
// entries with zeros = a gather), and every rank sorts the same list.
constexpr int kSelCap = 4096;      // candidates per (column, slot): what the histogram buffer holds
constexpr int kSelMaxWorld = 64;   // rows of the count buffer
// this rank's candidates of (col, slot): the entry of its own round-2 histogram at the digit the (global) step chose
CD_HD double sel_local_count(const FitScalars *sc, const double *local_hist, int col, int slot) {
    const uint64_t p0 = sc->sel_prefix[2 * col], p1 = sc->sel_prefix[2 * col + 1];
    if (slot == 1 && p0 == p1) return 0.0;  // the upper middle shares the lower one's candidates
    const uint64_t p = slot ? p1 : p0;
    const int hslot = (slot == 1 && (p0 >> 52) != (p1 >> 52)) ? 1 : 0;  // which round-2 histogram counted them
    return local_hist[((size_t)col * 2 + hslot) * kSelBins + (size_t)((p >> 40) & (kSelBins - 1))];
}
// offset of `rank`'s candidates of entry q (= 2*col + slot) and the total over ranks, from the all-reduced counts
CD_HD void sel_gather_layout(const double *cnt, int world, int rank, int nq, int q, double *base, double *total) {
    double b = 0, t = 0;
    for (int r = 0; r < world; r++) {
        const double c = cnt[(size_t)r * nq + q];
        if (r < rank) b += c;
        t += c;
    }
    *base = b;
    *total = t;
}

// ---- prior variance (estimateDispersionsPriorVar, closed-form branch) ---------------------------
CD_HD double trigamma_pos(double x) {
    double r = 0.0;
    while (x < 10.0) {
        r += 1.0 / (x * x);
        x += 1.0;
    }
    const double xi = 1.0 / x, x2 = xi * xi;
    double s = 691.0 / 2730.0 - x2 * (7.0 / 6.0);
    s = 5.0 / 66.0 - x2 * s;
    s = 1.0 / 30.0 - x2 * s;
    s = 1.0 / 42.0 - x2 * s;
    s = 1.0 / 30.0 - x2 * s;
    s = 1.0 / 6.0 - x2 * s;
    return r + xi * (1.0 + 0.5 * xi + x2 * s);
}
CD_HD void prior_var(FitScalars *sc, int S, int p, double prior_in) {
    const double v = sc->mad * sc->mad;
    sc->varLogDispEsts = v;
    sc->dispPriorVar = (prior_in == prior_in) ? prior_in : fmax(v - trigamma_pos((S - p) / 2.0), 0.25);
}

}  // namespace cd
