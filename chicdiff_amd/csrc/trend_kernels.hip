// trend_kernels.hip — the fit's global statistics between the gene-wise search and the MAP search.
//
//  * dispersion trend  alpha(mu) = a0 + a1/mu  — DESeq2 parametricDispersionFit + R glm.fit for
//    Gamma(link="identity"): one fused pass per IRLS step (deviance of
//    the current iterate + weighted-LS sums for the next), fixed-order reductions, and a state
//    machine that runs on the device (fit_state.h).  Single rank: ONE persistent launch with the
//    rows resident in LDS and a grid barrier per pass; sharded: one launch + one all-reduce of the
//    block partials + one reduce-and-step launch per pass;
//  * in the same persistent launch, the log residuals, their median and MAD (A3) by a radix or a
//    value-binned select, and the closed-form prior variance (A4);
//  * the local-regression trend (lf_*), and the simulation-matched prior variance for
//    d.f. <= 3 (prior_mc.h).
// The exact medians over all rows (radix select, size factors) are in global_kernels.hip.
#include "common.h"
#include "devmath.h"
#include "prior_mc.h"

namespace cd {

// ------------------------------------------------------------------------------------------
template <int K>
__device__ __forceinline__ void block_reduce_store(double (&v)[K], double *out) {
    __shared__ double red[K][4];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
    for (int k = 0; k < K; k++) {
        double x = v[k];
        for (int off = 32; off > 0; off >>= 1) x += __shfl_down(x, off);
        if (lane == 0) red[k][wave] = x;
    }
    __syncthreads();
    if (threadIdx.x < K) out[threadIdx.x] = (red[threadIdx.x][0] + red[threadIdx.x][1]) + (red[threadIdx.x][2] + red[threadIdx.x][3]);
}

// sums[k] = sum_b partials[b*K + k], fixed order (deterministic)
__global__ void reduce_partials_kernel(const double *partials, int nblk, int K, double *sums) {
    __shared__ double red[256];
    for (int k = 0; k < K; k++) {
        double acc = 0;
        for (int b = threadIdx.x; b < nblk; b += 256) acc += partials[(int64_t)b * K + k];
        red[threadIdx.x] = acc;
        __syncthreads();
        for (int s = 128; s > 0; s >>= 1) {
            if ((int)threadIdx.x < s) red[threadIdx.x] += red[threadIdx.x + s];
            __syncthreads();
        }
        if (threadIdx.x == 0) sums[k] = red[0];
        __syncthreads();
    }
}

// ------------------------------------------------------------------------------------------
// trend (state machine: fit_state.h)
__global__ void trend_init_kernel(FitWork w) { trend_init(w.sc); }

// One row's contribution to a trend pass (fit_state.h trend_row, which the CPU harness runs as written) with the device's
// lean arithmetic: x = 1/baseMean comes in ready, the two quotients become reciprocals (rcp: <= 1 ulp) and the
// logarithm the table-driven tlog — about 55 instructions instead of about 200 (five IEEE divisions and a library log),
// which was half of a pass of the persistent kernel at 2 M rows.
__device__ __forceinline__ void trend_row_dev(const FitScalars *sc, double x, double disp, double *v, const LogEntry *lt) {
    const double r = disp * rcp(fma(sc->coefs[1], x, sc->coefs[0]));
    if (!(r > 1e-4 && r < 15)) return;
    const double mu = fma(sc->b[1], x, sc->b[0]);
    if (!(mu > 0) || !isfinite(mu)) {
        v[7] += 1;
        return;
    }
    const double rmu = rcp(mu), q = disp * rmu;
    v[0] += -2.0 * (tlog(q, lt) - fma(-mu, rmu, q));  // Gamma deviance residual: log(y/mu) - (y - mu)/mu
    const double wt = rmu * rmu;                        // glm.fit weight for Gamma/identity
    v[1] += wt;
    v[2] += wt * x;
    v[3] += wt * x * x;
    v[4] += wt * disp;
    v[5] += wt * x * disp;
    v[6] += 1;
}
// A row of a speculative pass (fit_state.h trend_step_spec): v as above, and u, what the start pass of the next glm() call adds
// for this row if this pass converges.  That pass runs with coefs := b, so its filter ratio disp * rcp(fma(coefs[1], x, coefs[0]))
// is q, bit for bit, and its seven terms are the ones formed here — each is computed once and added to v, to u, or to both.  A row
// whose mu is not positive and finite never enters u: rcp(mu) is then negative, zero or NaN and q fails the filter, as in the real
// start pass, so u[7] stays zero.  Rows the current filter rejects (which return early above) are looked at here.
__device__ __forceinline__ void trend_row_spec_dev(const FitScalars *sc, double x, double disp, double *v, double *u, const LogEntry *lt) {
    const double r = disp * rcp(fma(sc->coefs[1], x, sc->coefs[0]));
    const bool in_v = r > 1e-4 && r < 15;
    const double mu = fma(sc->b[1], x, sc->b[0]);
    if (!(mu > 0) || !isfinite(mu)) {
        if (in_v) v[7] += 1;
        return;
    }
    const double rmu = rcp(mu), q = disp * rmu;
    const bool in_u = q > 1e-4 && q < 15;
    if (!in_v && !in_u) return;
    const double t0 = -2.0 * (tlog(q, lt) - fma(-mu, rmu, q));
    const double wt = rmu * rmu;
    const double t2 = wt * x, t3 = wt * x * x, t4 = wt * disp, t5 = wt * x * disp;
    if (in_v) { v[0] += t0; v[1] += wt; v[2] += t2; v[3] += t3; v[4] += t4; v[5] += t5; v[6] += 1; }
    if (in_u) { u[0] += t0; u[1] += wt; u[2] += t2; u[3] += t3; u[4] += t4; u[5] += t5; u[6] += 1; }
}

__global__ __launch_bounds__(256) void trend_pass_kernel(FitDims d, FitWork w, double minDisp) {
    __shared__ LogEntry s_lt[64];
    log_table_to_lds(s_lt);
    const FitScalars *sc = w.sc;
    if (sc->finished) return;
    double v[kTrendSums] = {0, 0, 0, 0, 0, 0, 0, 0};
    for (int64_t i = blockIdx.x * 256 + threadIdx.x; i < d.n; i += (int64_t)gridDim.x * 256) {
        if (w.allZero[i]) continue;
        const double y = w.dispGene[i];
        if (!(y > 100 * minDisp)) continue;  // useForFit <- dispGeneEst > 100*minDisp
        trend_row_dev(sc, 1.0 / w.baseMean[i], y, v, s_lt);
    }
    block_reduce_store<kTrendSums>(v, w.partials + (size_t)blockIdx.x * kTrendSums);
}

// one block: fixed-order sum of the block partials; with a single rank the same block also
// advances the state machine (with several ranks the sums are all-reduced first)
__global__ __launch_bounds__(256) void trend_reduce_kernel(FitWork w, int nblk, int do_step) {
    __shared__ double red[kTrendSums][4];
    double *sums = sums_of(w);
    if (w.sc->finished) return;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    for (int k = 0; k < kTrendSums; k++) {
        double acc = 0;
        for (int b = threadIdx.x; b < nblk; b += 256) acc += w.partials[(size_t)b * kTrendSums + k];
        for (int off = 32; off > 0; off >>= 1) acc += __shfl_down(acc, off);
        if (lane == 0) red[k][wave] = acc;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        for (int k = 0; k < kTrendSums; k++) sums[k] = (red[k][0] + red[k][1]) + (red[k][2] + red[k][3]);
        if (do_step) trend_step(w.sc, sums);
    }
}
__global__ void trend_step_kernel(FitWork w) { trend_step(w.sc, sums_of(w)); }

// ---- single-rank fast path: the whole trend fit in ONE persistent launch ------------------------------
// One 1024-thread workgroup per CU; each owns a contiguous block of rows and keeps their
// (baseMean, dispGeneEst) pairs in LDS (2 M rows = 125 KB per CU of the 160 KB), so the ~20 IRLS passes
// of glm.fit read HBM once instead of 20 times and need no kernel boundary: per pass every workgroup
// publishes 8 partial sums (16 in a speculative pass, see trend_row_spec_dev), a grid barrier (monotonic counter, agent-scope release/acquire, cdna guide
// G16) follows, and every workgroup adds the partials in the same fixed order and advances its own copy
// of the state machine (fit_state.h) — identical in all workgroups, no broadcast needed.
// The start pass of every glm() call after the first is not run where the pass before it, the converging one, was announced as
// speculative by the state machine and has summed the start pass's values on the side: 2 passes of 13 at 200 k x 8, 3 of 18 at
// 30 k x 4 (option "trend_speculate" = 0: every pass as before; same bits either way).
constexpr int kTpSums = 2 * kTrendSums;  // a workgroup's slot per pass: v[8], then u[8] of a speculative pass
constexpr int kTpBlocks = 256, kTpThreads = 1024, kTpCap = 8000, kTpMinRows = 2048;  // rows cached per workgroup (2 x 64 000 B of LDS)
// The exchange of the passes after the first (option "trend_exchange"; 0: every pass by the grid barrier, as pass 0).  What the
// barrier's two fences, its chain of arrivals and the re-read cost — 7-9 of a pass's ~19 us at 2 M rows — bought was only that a
// counter could vouch for data that travelled apart from it.  Here every 64-bit word vouches for itself (fit_state.h xchg_pack:
// tag = pass + 1 beside half a double), so nothing has to be ordered against anything:
//  * writer: thread t < nsums stores the two words of sum t, relaxed at agent scope — no fence, no counter, no wait;
//  * reader: wave k < nsums sums quantity k as before, lane l taking workgroups l, l + 64, ... in ascending order; it polls its
//    words, relaxed at agent scope, until each carries this pass's tag (xchg_accept, word by word: no order between two words is
//    assumed anywhere), then adds the doubles in that same order: the parent's tree, operand for operand, so every bit stays;
//  * layout: FitWork::xchg[pass parity][sum][workgroup][2] — a wave's poll is one contiguous run of 16 bytes per workgroup (the
//    flag barrier below had 256 x 256 polls on sixteen lines), in a buffer nobody else writes: no stale double can pass for a tag;
//  * stale words of an earlier launch are impossible, not improbable: the buffer lies behind FitWork::barrier and is zero-filled
//    with it by the one fill at the head of every pass of a fit — refits and the gathered route of sharded fits (which launches on
//    a copy of the same FitWork) included — and tag 0 is accepted by no pass;
//  * parity: a workgroup stores pass p + 2 into the buffer of pass p only after it has accepted every workgroup's words of p + 1
//    (its stores take their values from the state step, which takes its from those loads), and a workgroup stores p + 1 only after
//    it has accepted — finished reading — all of p.  So when a word of p is overwritten, every reader is done with it;
//  * a lane that waits kXchgSpins polls in vain (grid_sync's patience: a workgroup that never became resident) marks the workgroup
//    lost through LDS; it leaves, its peers run out in turn, failed = 3, and the host fits again with one launch per pass.  The
//    timeout cascades: the peers of the workgroup that left first find out only by waiting in vain for its words of the NEXT pass,
//    each for its own full patience, so the launch ends after about two patiences where a lost grid_sync ends after one;
// grid_sync stays where atomics and lists are published: pass 0 (which orders the zeroing of the MAD scratch by workgroup 0 before
// any workgroup's first MAD atomic), the MAD step and mad_select.  Its counters count those real barriers alone.
// One round of polls is 256 workgroups x 8 or 16 waves x 4 KB — 8 or 16 MB through the fabric, about 2 us, the price of the barrier
// route's re-read — so a round that cannot succeed is not free: it holds up the very stores everybody waits for.  A poll issued
// straight behind the workgroup's own stores always fails (the stores take longer than that to become visible, and the other
// workgroups are not all there yet), so the reader sleeps kXchgFirstSleep x 64 clocks first, ~0.9 us.  Measured in whole steps, six
// alternating runs each (profiles/r35_ab_variants.txt): without that sleep and s_sleep 2 between polls 3.230-3.248 ms at 2 M x 8
// (one run 3.423) against the barrier route's 3.247-3.256; 16 and 8: 3.187-3.209; 32 and 4: 3.167-3.183, and, medians of three runs, barrier
// route -> 32 and 4: 1.193 -> 1.155 ms at 250 k x 8, 0.697 -> 0.678 at 30 k x 4.
constexpr int kXchgSpins = 1 << 24, kXchgFirstSleep = 32, kXchgPollSleep = 4;
static_assert(kXchgBytes == 2 * kTpSums * kTpBlocks * 2 * 8 && kTpBlocks % 64 == 0, "trend exchange: layout of FitWork::xchg");

// Two-level grid barrier: workgroups arrive at one of 8 group counters (blockIdx % 8, i.e. one per XCD under
// round-robin dispatch — different cache lines, so the arrivals of different groups do not serialise behind one
// another), the last arrival of a group bumps the top counter, everybody polls the top counter.  256 atomics on
// one word cost ~10 us per barrier; this way the longest chain is 32 + 8.  `pass` counts the calls of a launch from 0, without gaps
// (the counters only ever grow): the kernel's nbar, not the number of the trend pass.
__device__ __forceinline__ bool grid_sync(unsigned int *top, unsigned int *groups, unsigned int pass) {
    __shared__ int ok;
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");  // this wave's stores have left
    __syncthreads();
    if (threadIdx.x == 0) {
        const unsigned int nblk = gridDim.x, g = blockIdx.x & 7u;
        const unsigned int ngroups = nblk < 8u ? nblk : 8u, gsize = (nblk - g + 7u) >> 3;
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "agent");
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        const unsigned int old = __hip_atomic_fetch_add(groups + g * 16u, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);  // 64-byte stride
        if (old + 1u == (pass + 1u) * gsize) {
            __builtin_amdgcn_fence(__ATOMIC_RELEASE, "agent");
            __hip_atomic_fetch_add(top, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        }
        const unsigned int target = (pass + 1u) * ngroups;
        int spins = 0;
        while (__hip_atomic_load(top, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) < target && spins < (1 << 24)) {
            __builtin_amdgcn_s_sleep(2);
            spins++;
        }
        ok = spins < (1 << 24);  // a bounded spin: a lost workgroup must not hang the device
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    }
    __syncthreads();
    return ok != 0;
}
// (Measured and dropped, round 4: a barrier by flags — workgroup b publishes `pass + 1` in flags[b], thread t of every workgroup
// polls flags[t]; no read-modify-write, no chain of arrivals.  Slower: 4.6-5.4 us per barrier instead of 3.3-3.8 at 122 workgroups,
// 12.8 instead of 5-6 at 256 — 256 x 256 polling loads per round trip swamp the path to the flags' home.  And the counters
// without the top level — arrivals by an atomic add nobody waits for, lanes 0..7 of every workgroup polling the eight group
// counters, so that no arrival depends on a returned count: workgroup 0 passes the barriers of the trend passes in 2.2 instead of
// 3.6 us (250 k rows) and 3.7 instead of 5-6 (2 M), but the barriers of the MAD's histogram rounds, where every workgroup arrives
// in a burst behind its global atomics, get slower by as much: launch 0.190 -> 0.188 ms at 250 k, 0.365 -> 0.380 at 2 M.
// Round 35: the trend's passes after the first do without this barrier altogether — their sums travel as self-tagged words
// ("exchange", above the kernel): workgroup 0's window from its sums to everybody's, stamps 12 -> 14, 6.0-9.3 -> 2.2-2.6 us at 2 M
// rows, 4.4-5.4 -> 1.8-2.2 at 250 k, 2.8-3.4 -> 1.7-1.8 at 30 k x 4, a whole pass 17.3-20.7 -> 11.1-13.9, 9.5-12.1 -> 6.5-8.9 and
// 6.7-9.6 -> 6.2-8.5 us (profiles/r35_trend_stamps.txt); the launch 305 -> 233 us at 2 M x 8.  The barrier stays for pass 0 and
// the MAD step.)

// Sum over the 64 lanes of a wave, result in lane 63, by DPP row shifts and row broadcasts (an inclusive scan: fixed order, no
// LDS round trips).  The eight sums of a trend pass through ds_bpermute shuffles were 48 dependent LDS trips per wave — with 16
// waves per workgroup 4-6 us of a 12-20 us pass (same stamps).
template <int CTRL, int ROW_MASK>
__device__ __forceinline__ double dpp_add(double x) {
    const int lo = __builtin_amdgcn_update_dpp(0, __double2loint(x), CTRL, ROW_MASK, 0xf, false);
    const int hi = __builtin_amdgcn_update_dpp(0, __double2hiint(x), CTRL, ROW_MASK, 0xf, false);
    return x + __hiloint2double(hi, lo);  // lanes without a source (or masked out) add +0.0
}
__device__ __forceinline__ double wave_sum_to_lane63(double x) {
    x = dpp_add<0x111, 0xf>(x);  // row_shr:1
    x = dpp_add<0x112, 0xf>(x);  // row_shr:2
    x = dpp_add<0x114, 0xf>(x);  // row_shr:4
    x = dpp_add<0x118, 0xf>(x);  // row_shr:8   -> lane 15 of every row of 16: the row's sum
    x = dpp_add<0x142, 0xa>(x);  // row_bcast:15 into rows 1 and 3
    x = dpp_add<0x143, 0xc>(x);  // row_bcast:31 into rows 2 and 3 -> lane 63: everything
    return x;
}

// ---- MAD of the log residuals inside the persistent trend kernel ------------------------------------------------------
// Round 3 followed the trend kernel with resid_kernel and two radix selects — 14 dependent launches and 4 fills that move 16 MB
// each and take 0.17 ms at 2 M rows, 0.11 ms at 250 k: pure launch latency.  The trend kernel has every row in LDS and a grid
// barrier at hand, so it goes on: residuals (written to w.resid as before), then for the median and for the median of the
// absolute deviations the same exact radix select — 12-bit digit histograms (LDS, then one global atomic per non-empty bin), a
// grid barrier, every workgroup picks the bins that hold the two middle ranks, next digit ... until at most kSelCap keys share
// the chosen prefix (after two rounds unless the data are massively tied), then the candidates are appended to a global list,
// one more barrier, and every workgroup sorts the same short list in LDS and reads the order statistics off it.  Exact, so the
// medians — and everything downstream — are the bits of the launches it replaces.
// Global scratch (w.hist, as 32-bit words, zeroed by the kernel): per select s in {median, absdev} and slot q in {lower, upper}
//   hist[s][round 0..5][q][4096], cnt[s][q], then 64-bit keys cand[s][q][kSelCap].
constexpr int kMadSortMax = 512;  // candidates per slot that are sorted rather than narrowed down by another round (<= kSelCap)
constexpr int kMadHistWords = 2 * 6 * 2 * kSelBins;
constexpr int kMadCntWords = 8;                                  // 2 x 2 counters (+ pad)
constexpr int kMadScratchWords = kMadHistWords + kMadCntWords;   // the radix select's words that must be zero
// ... then the value-binned route's (below): its histogram and vcnt[0] median candidates, [1] candidates of the MAD, [2] rows below
// the MAD's bracket, [3] population of |x - med|; all of it is zeroed by the kernel.  The candidate lists follow (8-byte aligned):
// the radix select's four of kSelCap keys, then the value route's two of kVbCap.
constexpr int kVbCntWords = 8;
constexpr int kMadZeroWords = kMadScratchWords + kVbBins + kVbCntWords;
constexpr int kVbPer = kVbBins / 1024, kVbList2 = 1024;  // bins per thread of the kernel; keys a narrowed list may hold
static_assert(kVbBins == kVbPer * 1024 && kMadZeroWords % 2 == 0 && kVbCap * 8 <= 64000, "value-binned select: layout");
struct MadArgs {
    int enabled;       // 0: the kernel stops after the trend (the host launches the separate MAD step)
    int S, p;
    double prior_in;   // NaN = estimate; the closed-form prior variance is finished here unless by_simulation
    int by_simulation; // residual d.f. <= 3: the host follows up with the residual histogram and prior_mc
    int speculate;     // the trend's passes may speculate (option "trend_speculate")
    int exchange;      // the trend's passes after the first hand their sums over as self-tagged words, no grid barrier (option "trend_exchange")
    int value_route;   // median and MAD by the value-binned select, three grid barriers instead of six (option "mad_select_route")
    int value_cap;     // ... keys a candidate list may hold (option "mad_value_cap": a test can force the radix select)
};

#ifdef CHICDIFF_MAD_STAMPS
#define MSTAMP(label) do { if (blockIdx.x == 0 && threadIdx.x == 0 && g_mad_n < 64) { g_mad_lab[g_mad_n] = (label); g_mad_t[g_mad_n++] = __builtin_amdgcn_s_memrealtime(); } } while (0)
__device__ unsigned long long g_mad_t0, g_mad_t[64];
__device__ int g_mad_lab[64], g_mad_n;
#else
#define MSTAMP(label)
#endif
#ifdef CHICDIFF_TREND_STAMPS  // diagnostic build only: where a pass of the persistent trend kernel spends its time (workgroup 0)
#define TSTAMP(label) do { if (blockIdx.x == 0 && threadIdx.x == 0 && g_tr_n < 160) { g_tr_lab[g_tr_n] = (label); g_tr_t[g_tr_n++] = __builtin_amdgcn_s_memrealtime(); } } while (0)
__device__ unsigned long long g_tr_t[160];
__device__ int g_tr_lab[160], g_tr_n;
#else
#define TSTAMP(label)
#endif
// wave-aggregated histogram update: lanes that hold the same digit add once (the first digit — sign and exponent — is shared by
// almost every key of a column, and 64 lanes adding 1 to one LDS word serialise)
__device__ __forceinline__ void hist_add(unsigned int *h, bool valid, unsigned int digit) {
    unsigned long long todo = __ballot(valid);
    const int lane = threadIdx.x & 63;
    for (int it = 0; it < 4 && todo; it++) {
        const int leader = __ffsll((long long)todo) - 1;
        const unsigned int dl = (unsigned int)__shfl((int)digit, leader);
        const unsigned long long same = __ballot(valid && digit == dl) & todo;
        if (lane == leader) atomicAdd(&h[dl], (unsigned int)__popcll(same));
        todo &= ~same;
    }
    if ((todo >> lane) & 1ull) atomicAdd(&h[digit], 1u);  // (digits of the later rounds differ from lane to lane)
}

// The order statistics wanted, read off a list of m <= 1024 keys in LDS by COUNTING instead of sorting it: P = 1024 / (m rounded
// up to a power of two) threads share one candidate, each counts the keys that come before it (smaller, or equal with a lower
// index) in its slice of the list, the P counts are added by shuffles, and the candidate whose count is a wanted rank is an answer.
__device__ __forceinline__ void lds_count_select(const uint64_t *buf, int m, int wantA, int wantB, uint64_t *sh_res /*[2]*/) {
    const int tid = threadIdx.x;
    int mp = 64;
    while (mp < m) mp <<= 1;
    const int P = kTpThreads / mp;  // 1 .. 16 threads per candidate, neighbouring lanes
    const int e = tid / P, part = tid - e * P;
    int before = 0;
    const uint64_t mine = e < m ? buf[e] : 0ull;
    if (e < m)
        for (int j = part; j < m; j += P) {
            const uint64_t o = buf[j];
            before += (o < mine || (o == mine && j < e)) ? 1 : 0;
        }
    for (int off = 1; off < P; off <<= 1) before += __shfl_xor(before, off);
    if (e < m && part == 0) {  // (ranks are distinct: exactly one candidate has each)
        if (before == wantA) sh_res[0] = mine;
        if (before == wantB) sh_res[1] = mine;
    }
    __syncthreads();
}

// One exact select over the keys key_fn(k) of this workgroup's rows; returns the two middle order statistics as keys.
// `sel` picks the scratch; s_a / s_b: two LDS histograms of kSelBins words; sortbuf: kSelCap 64-bit words (may alias them).
// Every workgroup executes the same barriers and reaches the same result.  Returns false if a grid barrier timed out.
template <class KeyFn>
__device__ bool mad_select(KeyFn key_fn, int64_t nrows_block, int sel, unsigned int *gscratch, unsigned int *s_a, unsigned int *s_b,
                           uint64_t *sortbuf, unsigned int *ctr, unsigned int *grp, unsigned int &pass, uint64_t (&result)[2], double &population) {
    __shared__ uint64_t sh_pre[2], sh_res[2];
    __shared__ double sh_rank[2], sh_pop;
    __shared__ unsigned int sh_cnt[2];
    __shared__ double sh_scan[kTpThreads / 64];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    unsigned int *ghist = gscratch + (size_t)sel * 6 * 2 * kSelBins;
    unsigned int *gcnt = gscratch + kMadHistWords + sel * 2;
    uint64_t *gcand = reinterpret_cast<uint64_t *>(gscratch + kMadZeroWords) + (size_t)sel * 2 * kSelCap;
    uint64_t p0 = 0, p1 = 0;
    double rank0 = 0, rank1 = 0;
    int fixed_hi = 64;  // bits [fixed_hi, 64) of the two prefixes are decided
    for (int r = 0; r < 6; r++) {
        const int shift = kSelShifts[r], bits = sel_bits(shift), nb = 1 << bits;
        const bool same = p0 == p1;
        for (int k = tid; k < kSelBins; k += kTpThreads) { s_a[k] = 0; s_b[k] = 0; }
        __syncthreads();
        const int64_t trips = (nrows_block + kTpThreads - 1) / kTpThreads;  // (every thread the same number: hist_add ballots)
        for (int64_t t = 0; t < trips; t++) {
            const int64_t k = t * kTpThreads + tid;
            uint64_t key = 0;
            const bool valid = k < nrows_block && key_fn(k, key);
            const unsigned int dig = (unsigned int)((key >> shift) & (uint64_t)(nb - 1));
            const bool m0 = valid && sel_match(key, p0, fixed_hi), m1 = valid && !same && !m0 && sel_match(key, p1, fixed_hi);
            hist_add(s_a, m0, dig);
            if (!same) hist_add(s_b, m1, dig);
        }
        __syncthreads();
        unsigned int *g0 = ghist + ((size_t)r * 2 + 0) * kSelBins, *g1 = g0 + kSelBins;
        for (int k = tid; k < nb; k += kTpThreads) {
            if (s_a[k]) atomicAdd(&g0[k], s_a[k]);
            if (!same && s_b[k]) atomicAdd(&g1[k], s_b[k]);
        }
        MSTAMP(1);
        if (!grid_sync(ctr, grp, pass++)) return false;
        MSTAMP(2);
        // every workgroup: pick, for each slot, the bin that holds its rank (fit_state.h sel_pick, parallel: per-thread partial
        // sums over 4 consecutive bins, a scan over the 1024 threads, the owning thread refines)
        for (int hsel = 0; hsel < (same ? 1 : 2); hsel++) {  // one scan per distinct histogram; both slots read theirs off it
            const unsigned int *g = hsel ? g1 : g0;
            const int per = (nb + kTpThreads - 1) / kTpThreads;  // 4 (1 in the last, 16-bin round)
            double mine[4] = {0, 0, 0, 0}, acc = 0;
            for (int q = 0; q < per; q++) {
                const int b = tid * per + q;
                mine[q] = b < nb ? (double)g[b] : 0.0;
                acc += mine[q];
            }
            double incl = acc;  // inclusive scan over the workgroup (counts: exact in fp64)
            for (int off = 1; off < 64; off <<= 1) {
                const double o = __shfl_up(incl, off);
                if (lane >= off) incl += o;
            }
            if (lane == 63) sh_scan[wave] = incl;
            __syncthreads();
            double before_wave = 0, total = 0;
            for (int q = 0; q < kTpThreads / 64; q++) {
                if (q < wave) before_wave += sh_scan[q];
                total += sh_scan[q];
            }
            incl += before_wave;
            if (r == 0 && tid == 0) sh_pop = total;
            const double before = incl - acc;
            const bool last_thread = tid == (nb - 1) / per;
            for (int slot = 0; slot < 2; slot++) {
                if ((slot == 1 && !same) != (hsel == 1)) continue;  // slot 1 reads the second histogram when the prefixes differ
                double rank = slot ? rank1 : rank0;
                if (r == 0) {  // the first histogram's total is the population: ranks of the two middles (R median())
                    const int64_t mi = (int64_t)total;
                    rank = slot ? (double)(mi / 2) : (double)((mi - 1) / 2);
                }
                if ((before <= rank && rank < incl) || (last_thread && rank >= incl && incl == total)) {
                    double cum = before;
                    int q = 0;
                    for (; q < per - 1 && tid * per + q < nb - 1; q++) {
                        if (cum + mine[q] > rank) break;
                        cum += mine[q];
                    }
                    const int b = tid * per + q;
                    sh_pre[slot] = (slot ? p1 : p0) | ((uint64_t)b << shift);
                    sh_rank[slot] = rank - cum;
                    sh_cnt[slot] = g[b];
                }
            }
            __syncthreads();
        }
        MSTAMP(3);
        p0 = sh_pre[0]; p1 = sh_pre[1];
        rank0 = sh_rank[0]; rank1 = sh_rank[1];
        fixed_hi = shift;
        population = sh_pop;
        const unsigned int c0 = sh_cnt[0], c1 = sh_cnt[1];
        __syncthreads();
        if (population <= 0) { result[0] = result[1] = 0; return true; }  // empty: the caller sees population 0
        if (shift == 0) { result[0] = p0; result[1] = p1; return true; }  // every bit decided
        // few enough keys share the prefixes: gather and sort.  (A further round costs ~14 us — two passes over LDS and a grid barrier
        // — and a bitonic sort of 4096 keys ~55 us, of 512 ~10 us: measured, profiles/r04_mad_in_kernel_stamps.txt)
        if (c0 <= (unsigned int)kMadSortMax && c1 <= (unsigned int)kMadSortMax) break;
    }
    // candidates -> global lists (order irrelevant: they are sorted), then every workgroup sorts the same lists
    const bool same = p0 == p1;
    for (int64_t k = tid; k < nrows_block; k += kTpThreads) {
        uint64_t key;
        if (!key_fn(k, key)) continue;
        int slot = -1;
        if (sel_match(key, p0, fixed_hi)) slot = 0;
        else if (!same && sel_match(key, p1, fixed_hi)) slot = 1;
        if (slot < 0) continue;
        const unsigned int pos = atomicAdd(&gcnt[slot], 1u);
        if (pos < (unsigned int)kSelCap) gcand[(size_t)slot * kSelCap + pos] = key;
    }
    MSTAMP(4);
    if (!grid_sync(ctr, grp, pass++)) return false;
    MSTAMP(5);
    // The order statistics wanted, read off each list by COUNTING instead of sorting it (round 4: a bitonic sort of ~100 keys cost
    // 4 us — 28 rounds of compare-exchange with a workgroup barrier each — and there are up to four lists per MAD): the list goes
    // to LDS and lds_count_select reads the ranks off it.  Lists longer than 512 keep the sort.
    for (int slot = 0; slot < 2; slot++) {
        const int hslot = (slot == 1 && !same) ? 1 : 0;
        const int m = (int)gcnt[hslot];
        MSTAMP(100 + m);
        if (slot == 1 && same) break;  // (both middles were read off the one list below)
        const int rkA = (int)(slot ? rank1 : rank0), rkB = same ? (int)rank1 : -1;
        const int wantA = rkA < m ? rkA : m - 1, wantB = rkB < 0 ? -1 : (rkB < m ? rkB : m - 1);
        __syncthreads();
        if (m <= kMadSortMax) {
            for (int e = tid; e < m; e += kTpThreads) sortbuf[e] = gcand[(size_t)hslot * kSelCap + e];
            __syncthreads();
            lds_count_select(sortbuf, m, wantA, wantB, sh_res);
            result[slot] = sh_res[0];
            if (wantB >= 0) result[1] = sh_res[1];
            continue;
        }
        int len = 64;
        while (len < m) len <<= 1;
        for (int e = tid; e < len; e += kTpThreads) sortbuf[e] = e < m ? gcand[(size_t)hslot * kSelCap + e] : ~0ull;
        __syncthreads();
        for (int k2 = 2; k2 <= len; k2 <<= 1)  // bitonic sort, ascending
            for (int j = k2 >> 1; j > 0; j >>= 1) {
                for (int e = tid; e < len; e += kTpThreads) {
                    const int q = e ^ j;
                    if (q > e) {
                        const uint64_t x = sortbuf[e], y = sortbuf[q];
                        const bool up = (e & k2) == 0;
                        if ((x > y) == up) { sortbuf[e] = y; sortbuf[q] = x; }
                    }
                }
                __syncthreads();
            }
        result[slot] = sortbuf[wantA];
        if (wantB >= 0) result[1] = sortbuf[wantB];
        __syncthreads();
    }
    MSTAMP(6);
    return true;
}

// ---- value-binned route of the MAD step (fit_state.h "value-binned select"): three grid barriers instead of six -------------
// Residual pass: every valid residual also goes into an LDS histogram over its VALUE, merged into a global one; barrier 1.  Every
// workgroup scans that histogram (vb_pick), the rows of the median's bin(s) go to one candidate list; barrier 2; every workgroup
// reads the two middle ranks off the list on its own.  With the median known the same histogram brackets the two middle values
// of |x - med| (vb_bracket); one more pass counts the rows below the bracket and lists those inside it, both by comparing
// |x - med| itself; barrier 3; every workgroup checks the counts (vb_check) and selects from the list.  A list that does not fit
// or a failed check sends that select to mad_select above: the decision comes from the histogram or from counters read behind a
// barrier, so every workgroup takes the same turn.

// LDS of the value route besides the freed row cache: second-level histogram, narrowed list, and a few words
struct VbShared {
    unsigned int sub[kVbSub];
    uint64_t list2[kVbList2];
    uint64_t res[2];
    unsigned int wave[16], n, base, pop, below;
    unsigned int total, pbin[2], pbelow[2], pcnt[2];  // lds_hist_pick: entries in all; per rank its bin, the entries before that bin, in it
    int ia, ib;                                       // vb_bracket_par
    double lo, hi;
};

// Over the histogram h[0 .. PER * 1024), thread t owning PER consecutive words: the total, and for two ranks the bin that holds
// each (fit_state.h cum_locate), the entries before that bin and in it — found by the thread that owns the bin, no search.
// middle: the ranks are the two middle ranks of the total (R median()) instead of rA, rB.  cumulate: h becomes its inclusive
// prefix sums.  A rank beyond the total leaves its pick at the last bin.
template <int PER>
__device__ __forceinline__ void lds_hist_pick(unsigned int *h, VbShared &sh, bool middle, unsigned int rA, unsigned int rB, bool cumulate) {
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    unsigned int mine[PER], acc = 0;
#pragma unroll
    for (int q = 0; q < PER; q++) {
        mine[q] = h[tid * PER + q];
        acc += mine[q];
    }
    unsigned int incl = acc;
    for (int off = 1; off < 64; off <<= 1) {
        const unsigned int o = __shfl_up(incl, off);
        if (lane >= off) incl += o;
    }
    if (lane == 63) sh.wave[wave] = incl;
    if (tid == 0) {
        sh.pbin[0] = sh.pbin[1] = PER * kTpThreads - 1;
        sh.pbelow[0] = sh.pbelow[1] = sh.pcnt[0] = sh.pcnt[1] = 0;
    }
    __syncthreads();
    unsigned int before = incl - acc, total = 0;
    for (int q = 0; q < kTpThreads / 64; q++) {
        if (q < wave) before += sh.wave[q];
        total += sh.wave[q];
    }
    if (tid == 0) sh.total = total;
    if (middle) {
        rA = total ? (total - 1) / 2 : 0;
        rB = total / 2;
    }
#pragma unroll
    for (int slot = 0; slot < 2; slot++) {
        const unsigned int r = slot ? rB : rA;
        if (before <= r && r - before < acc) {
            unsigned int c = before;
            int q = 0;
            for (; q < PER - 1; q++) {
                if (c + mine[q] > r) break;
                c += mine[q];
            }
            sh.pbin[slot] = tid * PER + q;
            sh.pbelow[slot] = c;
            sh.pcnt[slot] = mine[q];
        }
    }
    if (cumulate) {
        unsigned int run = before;
#pragma unroll
        for (int q = 0; q < PER; q++) {
            run += mine[q];
            h[tid * PER + q] = run;
        }
    }
    __syncthreads();
}

// fit_state.h vb_bracket by all threads at once (its two conditions are monotone in rho, so any search finds the same grid
// points): the 8 * kVbBins = 1024 x 120 steps of a quarter bin are cut into 1024 intervals, every thread tests the two ends of
// its own, and 120 threads then test the points inside the interval where the condition turns.  cum: inclusive prefix sums.
__device__ __forceinline__ void vb_bracket_par(const unsigned int *cum, double med, unsigned int rankA, unsigned int rankB, VbShared &sh) {
    constexpr int kStride = 8 * kVbBins / kTpThreads;  // 120
    const double step = 1.0 / (4.0 * kVbScale);
    const int tid = threadIdx.x;
    auto pa = [&](int p) { return p == 0 || (p <= 8 * kVbBins && vb_upper(cum, med, p * step) <= rankA); };  // lo: the largest p with pa
    auto pb = [&](int p) { return p <= 8 * kVbBins && vb_lower(cum, med, p * step) > rankB; };                 // hi: the smallest p with pb
    if (tid == 0) { sh.ia = 0; sh.ib = -1; }
    __syncthreads();
    const int p0 = tid * kStride, p1 = p0 + kStride;
    if (pa(p0) && !pa(p1)) sh.ia = p0;      // lo in [p0, p1)
    if (tid == kTpThreads - 1 && pa(p1)) sh.ia = p1;  // (a median far outside the bins: the last point qualifies)
    if (!pb(p0) && pb(p1)) sh.ib = p0;      // hi in (p0, p1]; none: no p has pb, hi = +inf
    __syncthreads();
    const int ia = sh.ia, ib = sh.ib;
    __syncthreads();
    if (tid < kStride) {
        const int q = ia + tid;
        if (pa(q) && (tid == kStride - 1 || !pa(q + 1))) sh.ia = q;
    } else if (tid >= 128 && tid < 128 + kStride && ib >= 0) {
        const int q = ib + 1 + (tid - 128);
        if (pb(q) && !pb(q - 1)) sh.ib = q;
    }
    __syncthreads();
    if (tid == 0) {
        sh.lo = sh.ia * step;
        sh.hi = sh.ib < 0 ? INFINITY : sh.ib * step;
    }
    __syncthreads();
}

// Ranks kA <= kB <= kA + 1 of the global list glist[0, m), m <= kVbCap, whose values lie (mostly) in [vlo, vlo + kVbSub / scale).
// The list goes to LDS; up to kMadSortMax keys are counted at once, a longer list is first narrowed to the second-level bin(s) of
// the two ranks.  false: more than kVbList2 keys share those bins (ties) — the same verdict in every workgroup.
__device__ bool vb_list_select(const uint64_t *glist, int m, double vlo, double scale, int kA, int kB, uint64_t *lst, VbShared &sh, uint64_t (&res)[2]) {
    const int tid = threadIdx.x;
    for (int e = tid; e < m; e += kTpThreads) lst[e] = glist[e];
    for (int k = tid; k < kVbSub; k += kTpThreads) sh.sub[k] = 0;
    if (tid == 0) sh.n = 0;
    __syncthreads();
    if (m <= kMadSortMax) {
        lds_count_select(lst, m, kA, kB, sh.res);
    } else {
        for (int e = tid; e < m; e += kTpThreads) atomicAdd(&sh.sub[vb_sub(value_of(lst[e]), vlo, scale)], 1u);
        __syncthreads();
        lds_hist_pick<kVbSub / kTpThreads>(sh.sub, sh, false, (unsigned int)kA, (unsigned int)kB, false);
        const int sA = (int)sh.pbin[0], sB = (int)sh.pbin[1], below = (int)sh.pbelow[0];
        const int m2 = (int)(sA == sB ? sh.pcnt[0] : sh.pcnt[0] + sh.pcnt[1]);  // (no key lies between two neighbouring ranks)
        if (m2 > kVbList2) return false;
        for (int e = tid; e < m; e += kTpThreads) {
            const int sb = vb_sub(value_of(lst[e]), vlo, scale);
            if (sb == sA || sb == sB) sh.list2[atomicAdd(&sh.n, 1u)] = lst[e];  // (no key between two neighbouring ranks: m2 in all)
        }
        __syncthreads();
        lds_count_select(sh.list2, m2, kA - below, kB - below, sh.res);
    }
    res[0] = sh.res[0];
    res[1] = sh.res[1];
    __syncthreads();
    return true;
}

// the global value histogram -> LDS
__device__ __forceinline__ void vb_load(const unsigned int *vhist, unsigned int *s_h) {
    for (int k = threadIdx.x; k < kVbBins; k += kTpThreads) s_h[k] = vhist[k];
    __syncthreads();
}

// Workgroup-aggregated append: the keys for which pred(k, key) holds go to an LDS stage first, one global atomic reserves their
// place in the list.  A workgroup with more than `cap` of them adds its count all the same (the list has overflowed then).
template <class Pred>
__device__ __forceinline__ void vb_append(Pred pred, int64_t nrows_block, uint64_t *stage, unsigned int cap, unsigned int *gcount, uint64_t *glist,
                                          VbShared &sh) {
    const int tid = threadIdx.x;
    if (tid == 0) sh.n = 0;
    __syncthreads();
    for (int64_t k = tid; k < nrows_block; k += kTpThreads) {
        uint64_t key;
        if (!pred(k, key)) continue;
        const unsigned int pos = atomicAdd(&sh.n, 1u);
        if (pos < cap) stage[pos] = key;
    }
    __syncthreads();
    const unsigned int n = sh.n;
    if (tid == 0 && n) sh.base = atomicAdd(gcount, n);
    __syncthreads();
    if (n && n <= cap) {
        const unsigned int base = sh.base;
        for (unsigned int e = tid; e < n; e += kTpThreads)
            if (base + e < cap) glist[base + e] = stage[e];
    }
}

__global__ __launch_bounds__(kTpThreads) void trend_persistent_kernel(FitDims d, FitWork w, double minDisp, MadArgs madargs) {
    const bool mad = madargs.enabled != 0;
    __shared__ double s_bm[kTpCap], s_y[kTpCap];  // 1 / baseMean and dispGeneEst (NaN = not used for the fit)
    __shared__ double red[kTpSums][16], tot[kTpSums];  // a pass's sums per wave; over all workgroups
    __shared__ int s_lost;                             // a lane of the exchange ran out of patience
    __shared__ FitScalars st;  // only the trend fields are used
    __shared__ LogEntry s_lt[64];
    __shared__ VbShared vsh;
    if (threadIdx.x < 64) s_lt[threadIdx.x] = kLogTable[threadIdx.x];  // (the barrier below covers it)
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int64_t per = (d.n + gridDim.x - 1) / gridDim.x;
    const int64_t r0 = (int64_t)blockIdx.x * per, r1 = (r0 + per < d.n) ? r0 + per : d.n;
    const int64_t nrows = r1 > r0 ? r1 - r0 : 0;
    const int ncache = nrows < kTpCap ? (int)nrows : kTpCap;
    for (int k = tid; k < ncache; k += kTpThreads) {
        const int64_t i = r0 + k;
        const double y = w.dispGene[i];
        s_bm[k] = 1.0 / w.baseMean[i];
        s_y[k] = w.allZero[i] ? NAN : y;  // (useForFit, y > 100 minDisp, is tested per pass: the MAD step below wants y >= 100 minDisp)
    }
    if (tid == 0) {
        trend_init(&st);
        s_lost = 0;
    }
    __syncthreads();
    unsigned int *ctr = reinterpret_cast<unsigned int *>(w.barrier), *grp = ctr + 16;  // top counter, then 8 group counters 64 B apart
    double *slots = w.partials;  // [2][gridDim.x][kTpSums], double-buffered by pass parity
    const bool speculate = madargs.speculate != 0, exchange = madargs.exchange != 0;
    const double thr = 100 * minDisp;
    // scratch of the MAD step (below): zeroed here, by one workgroup; the grid barrier of the first trend pass publishes it (every
    // launch runs at least one pass, and pass 0 crosses a real barrier under either exchange route)
    unsigned int *gscratch = reinterpret_cast<unsigned int *>(w.hist);
    if (mad && blockIdx.x == 0)
        for (int k = tid; k < kMadZeroWords; k += kTpThreads) gscratch[k] = 0;
    bool alive = true;
    unsigned int pass = 0;   // trend passes so far: the tag of the exchange's words and the parity of both routes' buffers
    unsigned int nbar = 0;   // grid_sync calls so far: its counters count real barriers only, consecutively
#ifdef CHICDIFF_TREND_STAMPS
    if (blockIdx.x == 0 && threadIdx.x == 0) g_tr_n = 0;
#endif
    TSTAMP(9);
    for (; pass < 11 * 27 + 16; pass++) {
        if (st.finished) break;
        TSTAMP(10);
        const bool spec = st.spec_next != 0;  // set by the step before this pass: the same in every workgroup
        const int nsums = spec ? kTpSums : kTrendSums;
        double v[kTrendSums] = {0, 0, 0, 0, 0, 0, 0, 0}, u[kTrendSums] = {0, 0, 0, 0, 0, 0, 0, 0};
        if (spec) {
            for (int k = tid; k < ncache; k += kTpThreads) {
                const double y = s_y[k];
                if (y > thr) trend_row_spec_dev(&st, s_bm[k], y, v, u, s_lt);
            }
            for (int64_t i = r0 + kTpCap + tid; i < r1; i += kTpThreads) {
                const double y = w.dispGene[i];
                if (!w.allZero[i] && (y > 100 * minDisp)) trend_row_spec_dev(&st, 1.0 / w.baseMean[i], y, v, u, s_lt);
            }
        } else {
            for (int k = tid; k < ncache; k += kTpThreads) {
                const double y = s_y[k];
                if (y > thr) trend_row_dev(&st, s_bm[k], y, v, s_lt);  // (NaN fails)
            }
            for (int64_t i = r0 + kTpCap + tid; i < r1; i += kTpThreads) {  // rows beyond the LDS cache stream from HBM
                const double y = w.dispGene[i];
                if (!w.allZero[i] && (y > 100 * minDisp)) trend_row_dev(&st, 1.0 / w.baseMean[i], y, v, s_lt);
            }
        }
        TSTAMP(11);
#pragma unroll
        for (int k = 0; k < kTrendSums; k++) {
            const double x = wave_sum_to_lane63(v[k]);
            if (lane == 63) red[k][wave] = x;
        }
        if (spec) {  // (u through the same wave sum, workgroup sum and partial sum as v: the summation tree of a start pass)
#pragma unroll
            for (int k = 0; k < kTrendSums; k++) {
                const double x = wave_sum_to_lane63(u[k]);
                if (lane == 63) red[kTrendSums + k][wave] = x;
            }
        }
        __syncthreads();
        if (!(exchange && pass > 0)) {
            // publish, grid barrier, re-read: pass 0 always (its barrier also publishes the MAD scratch zeroed above), and every
            // pass with "trend_exchange" = 0
            double *mine = slots + ((size_t)(pass & 1) * gridDim.x + blockIdx.x) * kTpSums;
            if (tid < nsums) {
                double acc = 0;
                for (int q = 0; q < kTpThreads / 64; q++) acc += red[tid][q];
                mine[tid] = acc;
            }
            TSTAMP(12);
            alive = grid_sync(ctr, grp, nbar++);
            TSTAMP(13);
            if (!alive) break;
            // every workgroup: fixed-order sum of all partials (wave k sums quantity k: 64 lanes x strided
            // partials, then a shuffle tree — the same order in every workgroup), then the same state-machine step
            const double *all = slots + (size_t)(pass & 1) * gridDim.x * kTpSums;
            if (wave < nsums) {
                double acc = 0;
                for (unsigned int b = lane; b < gridDim.x; b += 64) acc += all[(size_t)b * kTpSums + wave];
                acc = wave_sum_to_lane63(acc);
                if (lane == 63) tot[wave] = acc;
            }
            __syncthreads();
        } else {
            // the exchange (above the kernel): thread t stores the two words of sum t, wave k polls and adds sum k of every workgroup
            const unsigned int tag = pass + 1u, nblk = gridDim.x;
            unsigned long long *xbuf = w.xchg + (size_t)(pass & 1) * kTpSums * kTpBlocks * 2;
            if (tid < nsums) {
                double acc = 0;
                for (int q = 0; q < kTpThreads / 64; q++) acc += red[tid][q];
                uint64_t lo, hi;
                xchg_pack(acc, tag, &lo, &hi);
                unsigned long long *mine = xbuf + ((size_t)tid * kTpBlocks + blockIdx.x) * 2;
                __hip_atomic_store(mine, (unsigned long long)lo, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                __hip_atomic_store(mine + 1, (unsigned long long)hi, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            }
            TSTAMP(12);
            if (wave < nsums) {
                unsigned long long *src = xbuf + (size_t)wave * kTpBlocks * 2;  // this wave's poll: one contiguous run of nblk x 16 bytes
                constexpr int kStrides = kTpBlocks / 64;
                uint64_t lo[kStrides], hi[kStrides];
                bool ready = true;
                __builtin_amdgcn_s_sleep(kXchgFirstSleep);  // (no word can have arrived yet: see kXchgFirstSleep)
#pragma unroll
                for (int j = 0; j < kStrides; j++) {
                    const unsigned int b = lane + 64u * j;
                    lo[j] = hi[j] = 0;
                    if (b < nblk) {
                        lo[j] = __hip_atomic_load(src + 2 * b, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                        hi[j] = __hip_atomic_load(src + 2 * b + 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                        ready = ready && xchg_accept(lo[j], tag) && xchg_accept(hi[j], tag);
                    }
                }
                int spins = 0;
                while (!ready && spins < kXchgSpins) {  // only the lanes with a word missing, and only for those words
                    __builtin_amdgcn_s_sleep(kXchgPollSleep);
                    spins++;
                    ready = true;
#pragma unroll
                    for (int j = 0; j < kStrides; j++) {
                        const unsigned int b = lane + 64u * j;
                        if (b < nblk) {
                            if (!xchg_accept(lo[j], tag)) lo[j] = __hip_atomic_load(src + 2 * b, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                            if (!xchg_accept(hi[j], tag)) hi[j] = __hip_atomic_load(src + 2 * b + 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                            ready = ready && xchg_accept(lo[j], tag) && xchg_accept(hi[j], tag);
                        }
                    }
                }
                if (!ready) s_lost = 1;  // a bounded spin, as grid_sync's: a lost workgroup must not hang the device
                double acc = 0;          // the parent's tree, operand for operand: workgroups lane, lane + 64, ... in ascending order
#pragma unroll
                for (int j = 0; j < kStrides; j++)
                    if (lane + 64u * j < nblk) acc += xchg_unpack(lo[j], hi[j]);
                acc = wave_sum_to_lane63(acc);
                if (lane == 63) tot[wave] = acc;
            }
            TSTAMP(13);
            __syncthreads();
            alive = s_lost == 0;
            if (!alive) break;
        }
        TSTAMP(14);
        if (tid == 0) {
            double sv[kTrendSums], su[kTrendSums];  // (su is stale unless the pass speculated: not looked at then)
#pragma unroll
            for (int k = 0; k < kTrendSums; k++) { sv[k] = tot[k]; su[k] = tot[kTrendSums + k]; }
            if (spec) trend_step_spec(&st, sv, su, speculate);
            else trend_step_spec(&st, sv, nullptr, speculate);
        }
        __syncthreads();
        TSTAMP(15);
    }
    TSTAMP(16);
    // ---- MAD of the log residuals around the trend (estimateDispersionsFit's varLogDispEsts), see mad_select above --------
    double med = NAN, madv = NAN, nres = 0;
    if (mad && alive) {
#ifdef CHICDIFF_MAD_STAMPS
        if (blockIdx.x == 0 && threadIdx.x == 0) { g_mad_t0 = __builtin_amdgcn_s_memrealtime(); g_mad_n = 0; }
#endif
        const double c0 = st.coefs[0], c1 = st.coefs[1];
        const bool vroute = madargs.value_route != 0;
        const unsigned int vcap = (unsigned int)madargs.value_cap;
        // the freed 1 / baseMean cache holds the selects' LDS histograms, staged candidates and the lists being searched
        unsigned int *s_h = reinterpret_cast<unsigned int *>(s_bm);
        unsigned int *vhist = gscratch + kMadScratchWords, *vcnt = vhist + kVbBins;
        uint64_t *vcand = reinterpret_cast<uint64_t *>(gscratch + kMadZeroWords) + (size_t)4 * kSelCap;  // two lists of kVbCap keys
        if (vroute) {
            for (int k = tid; k < kVbBins; k += kTpThreads) s_h[k] = 0;
            __syncthreads();
        }
        // residuals as resid_kernel forms them (same expressions: same bits), to w.resid and — cached rows — over y in LDS
        for (int64_t k = tid; k < nrows; k += kTpThreads) {
            const int64_t i = r0 + k;
            const double y = k < ncache ? s_y[k] : (w.allZero[i] ? NAN : w.dispGene[i]);
            double r = NAN;
            if (y >= thr) r = log(y) - log(c0 + c1 / w.baseMean[i]);
            w.resid[i] = r;
            if (k < ncache) s_y[k] = r;
            if (vroute && r == r) atomicAdd(&s_h[vb_bin(r)], 1u);
        }
        __syncthreads();
        MSTAMP(0);
        unsigned int *s_a = reinterpret_cast<unsigned int *>(s_bm), *s_b = s_a + kSelBins;
        uint64_t *sortbuf = reinterpret_cast<uint64_t *>(s_bm);
        const double *resid_g = w.resid + r0;
        uint64_t res[2];
        double pop = 0;
        auto key_resid = [&](int64_t k, uint64_t &key) {
            const double x = k < ncache ? s_y[k] : resid_g[k];
            if (x != x) return false;
            key = key_of(x);
            return true;
        };
        bool med_done = false, mad_done = false, empty = false;
        VbPick pk = {};
        if (vroute) {
            for (int k = tid; k < kVbBins; k += kTpThreads)
                if (s_h[k]) atomicAdd(&vhist[k], s_h[k]);
            MSTAMP(21);
            alive = grid_sync(ctr, grp, nbar++);
            MSTAMP(22);
            if (alive) {
                vb_load(vhist, s_h);
                lds_hist_pick<kVbPer>(s_h, vsh, true, 0u, 0u, false);  // fit_state.h vb_pick; (its last barrier: the stage below overwrites the histogram)
                pk.pop = vsh.total;
                pk.rankA = pk.pop ? (pk.pop - 1) / 2 : 0;
                pk.rankB = pk.pop / 2;
                pk.binA = (int)vsh.pbin[0];
                pk.binB = (int)vsh.pbin[1];
                pk.below = vsh.pbelow[0];
                pk.count = pk.binA == pk.binB ? vsh.pcnt[0] : vsh.pcnt[0] + vsh.pcnt[1];
                empty = pk.pop == 0;
                MSTAMP(23);
                if (!empty && pk.count <= vcap) {
                    const int binA = pk.binA, binB = pk.binB;
                    auto in_bins = [&](int64_t k, uint64_t &key) {
                        const double x = k < ncache ? s_y[k] : resid_g[k];
                        if (x != x) return false;
                        const int b = vb_bin(x);
                        if (b != binA && b != binB) return false;
                        key = key_of(x);
                        return true;
                    };
                    vb_append(in_bins, nrows, sortbuf, vcap, &vcnt[0], vcand, vsh);
                    MSTAMP(24);
                    alive = grid_sync(ctr, grp, nbar++);
                    MSTAMP(25);
                    if (alive && vcnt[0] == pk.count) {
                        const double vlo = (double)binA / kVbScale - kVbOffset, scale = (double)kVbSub * kVbScale / (double)(binB + 1 - binA);
                        med_done = vb_list_select(vcand, (int)pk.count, vlo, scale, (int)(pk.rankA - pk.below), (int)(pk.rankB - pk.below), sortbuf, vsh, res);
                        pop = (double)pk.pop;
                    }
                    MSTAMP(26);
                }
            }
        }
        if (alive && !empty && !med_done) alive = mad_select(key_resid, nrows, 0, gscratch, s_a, s_b, sortbuf, ctr, grp, nbar, res, pop);
        if (alive) {
            nres = pop;
            med = pop > 0 ? (value_of(res[0]) + value_of(res[1])) / 2.0 : NAN;  // R median(): mean of the two middles
            const double m0 = med;
            auto key_absdev = [&](int64_t k, uint64_t &key) {
                double x = k < ncache ? s_y[k] : resid_g[k];
                if (x != x) return false;
                x = fabs(x - m0);
                if (x != x) return false;
                key = key_of(x);
                return true;
            };
            if (vroute && !empty && pop > 0) {
                vb_load(vhist, s_h);
                lds_hist_pick<kVbPer>(s_h, vsh, true, 0u, 0u, true);
                vb_bracket_par(s_h, m0, pk.rankA, pk.rankB, vsh);  // (its last barrier: the stage below overwrites the histogram)
                if (tid == 0) { vsh.pop = 0; vsh.below = 0; }
                const double lo = vsh.lo, hi = vsh.hi;
                MSTAMP(27);
                // every row is classified by |x - med| itself: counted below the bracket, listed inside it, ignored above
                unsigned int npop = 0, nbelow = 0;
                auto in_bracket = [&](int64_t k, uint64_t &key) {
                    if (!key_absdev(k, key)) return false;
                    const double a = value_of(key);
                    npop++;
                    if (a < lo) nbelow++;
                    return a >= lo && a < hi;
                };
                vb_append(in_bracket, nrows, sortbuf, vcap, &vcnt[1], vcand + kVbCap, vsh);
                for (int off = 32; off > 0; off >>= 1) {
                    npop += __shfl_down(npop, off);
                    nbelow += __shfl_down(nbelow, off);
                }
                if (lane == 0 && npop) atomicAdd(&vsh.pop, npop);
                if (lane == 0 && nbelow) atomicAdd(&vsh.below, nbelow);
                __syncthreads();
                if (tid == 0 && vsh.pop) atomicAdd(&vcnt[3], vsh.pop);
                if (tid == 0 && vsh.below) atomicAdd(&vcnt[2], vsh.below);
                MSTAMP(28);
                alive = grid_sync(ctr, grp, nbar++);
                MSTAMP(29);
                if (alive) {
                    uint32_t kA = 0, kB = 0;
                    if (vb_check(vcnt[3], vcnt[2], vcnt[1], vcap, &kA, &kB)) {
                        const double scale = (double)kVbSub / (hi - lo);  // (0 for hi = +inf: a longer list is then not narrowed but refused)
                        mad_done = vb_list_select(vcand + kVbCap, (int)vcnt[1], lo, scale, (int)kA, (int)kB, sortbuf, vsh, res);
                        pop = (double)vcnt[3];
                    }
                }
                MSTAMP(30);
            }
            if (alive && !mad_done) alive = mad_select(key_absdev, nrows, 1, gscratch, s_a, s_b, sortbuf, ctr, grp, nbar, res, pop);
            if (alive) madv = 1.4826 * (pop > 0 ? (value_of(res[0]) + value_of(res[1])) / 2.0 : NAN);  // R mad(): constant 1.4826
        }
    }
    if (blockIdx.x == 0 && tid == 0) {
        FitScalars *sc = w.sc;
        sc->coefs[0] = st.coefs[0]; sc->coefs[1] = st.coefs[1];
        sc->b[0] = st.b[0]; sc->b[1] = st.b[1];
        sc->devold = st.devold;
        sc->inner_it = st.inner_it; sc->outer_it = st.outer_it; sc->phase = st.phase;
        sc->conv = st.conv;
        sc->failed = alive ? (st.finished ? st.failed : 2) : 3;  // 3: grid barrier timed out
        sc->finished = 1;
#ifdef CHICDIFF_TREND_STAMPS
        for (int q = 0; q < g_tr_n; q++) printf("  trend stamp %3d %8.2f us\n", g_tr_lab[q], (double)(g_tr_t[q] - g_tr_t[0]) / 100.0);
#endif
#ifdef CHICDIFF_MAD_STAMPS
        for (int q = 0; q < g_mad_n; q++) printf("  mad stamp %3d %8.2f us\n", g_mad_lab[q], (double)(g_mad_t[q] - g_mad_t0) / 100.0);
#endif
        if (mad && alive) {
            sc->med = med;
            sc->nres = nres;
            sc->mad = madv;
            if (!madargs.by_simulation) prior_var(sc, madargs.S, madargs.p, madargs.prior_in);  // (else prior_mc_kernel follows)
        }
    }
}
// sharded fits: this rank's slice of the rows the trend is fitted to, written into the all-ranks arrays (zero elsewhere; the
// sum-all-reduce that follows is then an all-gather).  y = NaN marks an all-zero row.
__global__ __launch_bounds__(256) void trend_gather_kernel(FitDims d, FitWork w, double minDisp, double *xg, double *yg) {
    for (int64_t i = blockIdx.x * 256 + threadIdx.x; i < d.n; i += (int64_t)gridDim.x * 256) {
        const double y = w.dispGene[i];
        xg[i] = w.baseMean[i];
        yg[i] = w.allZero[i] ? NAN : y;  // (the trend kernel applies useForFit itself; the MAD of the residuals wants y >= 100 minDisp)
    }
}
void launch_trend_gather(FitDims d, FitWork w, Opts o, double *xg, double *yg, hipStream_t st) {
    trend_gather_kernel<<<kRedBlocks, 256, 0, st>>>(d, w, o.minDisp, xg, yg);
}
__global__ __launch_bounds__(256) void trend_compact_kernel(GatherLayout gl, const double *__restrict__ recv, double *__restrict__ xg,
                                                            double *__restrict__ yg) {
    const int r = blockIdx.y;
    const int64_t cnt = gl.off[r + 1] - gl.off[r];
    const double *src = recv + (int64_t)r * gl.block;
    for (int64_t i = blockIdx.x * 256 + threadIdx.x; i < cnt; i += (int64_t)gridDim.x * 256) {
        xg[gl.off[r] + i] = src[i];
        yg[gl.off[r] + i] = src[gl.maxn + i];
    }
}
void launch_trend_compact(const GatherLayout &gl, const double *recv, double *xg, double *yg, hipStream_t st) {
    int64_t bx = (gl.maxn + 255) / 256;
    if (bx > 2048 / gl.world) bx = 2048 / gl.world;
    if (bx < 1) bx = 1;
    trend_compact_kernel<<<dim3((unsigned)bx, (unsigned)gl.world), 256, 0, st>>>(gl, recv, xg, yg);
}
__global__ void poke_kernel(int32_t *p, int32_t v) { *p = v; }
void launch_poke(int32_t *p, int32_t v, hipStream_t st) { poke_kernel<<<1, 1, 0, st>>>(p, v); }
__global__ void flag_to_double_kernel(const int32_t *flag, double *out) { *out = *flag ? 1.0 : 0.0; }
void launch_flag_to_double(const int32_t *flag, double *out, hipStream_t st) { flag_to_double_kernel<<<1, 1, 0, st>>>(flag, out); }
int trend_persistent_blocks() { return kTpBlocks; }
void launch_trend_persistent(FitDims d, FitWork w, Opts o, hipStream_t st, bool with_mad) {
    // (the barrier counters AND the exchange's words, FitWork::xchg, were zeroed with the fit's scalars, and the trend runs once per
    // fill: a second launch of this kernel behind the same fill would find the counters advanced and, in xchg, words that carry the
    // tags of its own passes — stale sums it would accept.  Whoever launches it twice in one fit_pass must clear both in between)
    // as few workgroups as keep every row LDS-resident: the pass time is the grid barrier plus the all-partials sum,
    // both of which grow with the number of workgroups (small fits are latency-bound by these ~20 passes)
    // rows per workgroup: at most kTpCap (LDS), at least ~2 per thread — with 8 per thread the row loop (4 us) was as long
    // as the grid barrier of a small fit, with 2 it is 1 us and the barrier of the 4x larger grid costs less than that saved
    int64_t blocks = (d.n + kTpMinRows - 1) / kTpMinRows;
    if (blocks < 1) blocks = 1;
    if (blocks > kTpBlocks) blocks = kTpBlocks;
    // fewer on request: several fits sharing one GPU (the one-GPU rehearsal of a sharded fit) must keep ALL their trend kernels'
    // workgroups resident at once, or the grid barriers time out; rows beyond the LDS cache stream from HBM / L2
    if (o.trend_blocks > 0 && blocks > o.trend_blocks) blocks = o.trend_blocks;
    MadArgs m{};
    m.enabled = with_mad ? 1 : 0;
    m.S = d.S;
    m.p = d.p;
    m.prior_in = o.dispPriorVarIn;
    m.by_simulation = (!(o.dispPriorVarIn == o.dispPriorVarIn) && d.S - d.p <= 3 && d.S > d.p) ? 1 : 0;
    m.speculate = o.trend_speculate ? 1 : 0;
    m.exchange = o.trend_exchange ? 1 : 0;
    m.value_route = o.mad_route ? 1 : 0;
    m.value_cap = (o.mad_value_cap > 0 && o.mad_value_cap < kVbCap) ? o.mad_value_cap : kVbCap;
    trend_persistent_kernel<<<(unsigned)blocks, kTpThreads, 0, st>>>(d, w, o.minDisp, m);
}

void launch_trend_init(FitDims, FitWork w, Opts, hipStream_t st) { trend_init_kernel<<<1, 1, 0, st>>>(w); }
constexpr int kTrendBlocks = 512;
int trend_blocks() { return kTrendBlocks; }
void launch_trend_pass(FitDims d, FitWork w, Opts o, hipStream_t st, bool fused_step) {
    trend_pass_kernel<<<kTrendBlocks, 256, 0, st>>>(d, w, o.minDisp);
    if (fused_step) trend_reduce_kernel<<<1, 256, 0, st>>>(w, kTrendBlocks, 1);
}
void launch_trend_step(FitDims, FitWork w, Opts, hipStream_t st) { trend_reduce_kernel<<<1, 256, 0, st>>>(w, kTrendBlocks, 1); }

// residuals of log gene-wise estimates around the trend (rows with dispGeneEst >= 100*minDisp)
__global__ __launch_bounds__(256) void resid_kernel(FitDims d, FitWork w, double minDisp) {
    const double c0 = w.sc->coefs[0], c1 = w.sc->coefs[1];
    const bool local = w.sc->trend_local != 0;
    for (int64_t i = blockIdx.x * 256 + threadIdx.x; i < d.n; i += (int64_t)gridDim.x * 256) {
        double r = NAN;
        if (!w.allZero[i]) {
            const double y = w.dispGene[i];
            if (y >= 100 * minDisp) r = log(y) - log(local ? w.dispFit[i] : c0 + c1 / w.baseMean[i]);
        }
        w.resid[i] = r;
    }
}
void launch_dispfit_resid(FitDims d, FitWork w, Opts o, hipStream_t st) {
    resid_kernel<<<kRedBlocks, 256, 0, st>>>(d, w, o.minDisp);
}

// ---- local-regression trend: DESeq2 localDispersionFit = locfit(log disp ~ log mean, weights = mean) with locfit's
// defaults (alpha = 0.7 nearest-neighbour bandwidth, local quadratic, tricube kernel, rbox(cut = 0.8) tree, Hermite
// interpolation) — DESeq2's own substitute when the parametric trend fails, or fitType = "local" on request.  A handful
// of vertices (about ten), each needing one order statistic (the k-th smallest |x_i - x_v|: a byte-wise radix select,
// eight histogram rounds) and eight weighted sums over the rows; the tree itself grows on the host (api.hip,
// local_trend_fit).  Every statistic is a sum over rows, so the sharded path all-reduces it like the others.  Rare
// path: clarity over speed.  Rows in the fit: dispGeneEst > 100 minDisp (useForFit), x = log baseMean.
__device__ __forceinline__ bool lf_row(const FitWork &w, int64_t i, double minDisp, double &x) {
    if (w.allZero[i] || !(w.dispGene[i] > 100 * minDisp)) return false;
    x = log(w.baseMean[i]);
    return true;
}
// hist[b] += rows whose key (of x, or of |x - xv|) agrees with `prefix` above bit shift + 8 and has byte b at `shift`
__global__ __launch_bounds__(256) void lf_hist_kernel(FitDims d, FitWork w, double minDisp, int use_dist, double xv, uint64_t prefix, int shift,
                                                      double *hist) {
    __shared__ unsigned int h[256];
    h[threadIdx.x] = 0;
    __syncthreads();
    for (int64_t i = blockIdx.x * 256 + threadIdx.x; i < d.n; i += (int64_t)gridDim.x * 256) {
        double x;
        if (!lf_row(w, i, minDisp, x)) continue;
        const uint64_t key = key_of(use_dist ? fabs(x - xv) : x);
        if (shift < 56 && (key >> (shift + 8)) != (prefix >> (shift + 8))) continue;
        atomicAdd(&h[(key >> shift) & 255], 1u);
    }
    __syncthreads();
    if (h[threadIdx.x]) atomicAdd(&hist[threadIdx.x], (double)h[threadIdx.x]);  // integer counts: exact in any order
}
// partial sums of w K(u) dx^q (q = 0..4) and w K(u) y dx^q (q = 0..2) per block; lf_sums_finish adds them in a fixed order
__global__ __launch_bounds__(256) void lf_sums_kernel(FitDims d, FitWork w, double minDisp, double xv, double h, double *partials) {
    __shared__ double red[256];
    double v[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    for (int64_t i = blockIdx.x * 256 + threadIdx.x; i < d.n; i += (int64_t)gridDim.x * 256) {
        double x;
        if (!lf_row(w, i, minDisp, x)) continue;
        const double dx = x - xv, u = fabs(dx) / h;
        if (u >= 1.0) continue;
        const double c = 1.0 - u * u * u, y = log(w.dispGene[i]);
        double p = w.baseMean[i] * (c * c * c);
        for (int q = 0; q < 5; q++) {
            v[q] += p;
            if (q < 3) v[5 + q] += p * y;
            p *= dx;
        }
    }
    for (int k = 0; k < 8; k++) {
        red[threadIdx.x] = v[k];
        __syncthreads();
        for (int s = 128; s > 0; s >>= 1) {
            if ((int)threadIdx.x < s) red[threadIdx.x] += red[threadIdx.x + s];
            __syncthreads();
        }
        if (threadIdx.x == 0) partials[(size_t)blockIdx.x * 8 + k] = red[0];
        __syncthreads();
    }
}
__global__ void lf_sums_finish_kernel(const double *partials, int nblocks, double *out) {
    const int k = threadIdx.x;
    if (k >= 8) return;
    double s = 0;
    for (int b = 0; b < nblocks; b++) s += partials[(size_t)b * 8 + k];
    out[k] = s;
}
// dispFit = exp(predict(fit, log baseMean)) for every row with counts; marks the trend as local
__global__ __launch_bounds__(256) void lf_eval_kernel(FitDims d, FitWork w, LfVerts v) {
    if (blockIdx.x == 0 && threadIdx.x == 0) {
        w.sc->trend_local = 1;
        w.sc->coefs[0] = w.sc->coefs[1] = NAN;
        w.sc->failed = 0;
        w.sc->finished = 1;
    }
    for (int64_t i = blockIdx.x * 256 + threadIdx.x; i < d.n; i += (int64_t)gridDim.x * 256) {
        if (w.allZero[i]) continue;
        const double x = log(w.baseMean[i]);
        int j = 0;
        while (j + 2 < v.nv && x >= v.x[j + 1]) j++;  // the cell a descent with "left when x < midpoint" ends in
        const double z = v.x[j + 1] - v.x[j], t = (x - v.x[j]) / z;
        double p0, p1, p2, p3;  // locfit hermite2: cubic inside the cell, the end vertex's line outside the data range
        if (t < 0) { p0 = 1; p1 = 0; p2 = t; p3 = 0; }
        else if (t > 1) { p0 = 0; p1 = 1; p2 = 0; p3 = t - 1; }
        else { p1 = t * t * (3 - 2 * t); p0 = 1 - p1; p2 = t * (1 - t) * (1 - t); p3 = t * t * (t - 1); }
        w.dispFit[i] = exp(p0 * v.f[j] + p1 * v.f[j + 1] + (p2 * v.d[j] + p3 * v.d[j + 1]) * z);
    }
}
void launch_lf_hist(FitDims d, FitWork w, Opts o, int use_dist, double xv, uint64_t prefix, int shift, double *hist, hipStream_t st) {
    (void)hipMemsetAsync(hist, 0, sizeof(double) * 256, st);
    lf_hist_kernel<<<kRedBlocks, 256, 0, st>>>(d, w, o.minDisp, use_dist, xv, prefix, shift, hist);
}
void launch_lf_sums(FitDims d, FitWork w, Opts o, double xv, double h, double *partials, double *out8, hipStream_t st) {
    lf_sums_kernel<<<kRedBlocks, 256, 0, st>>>(d, w, o.minDisp, xv, h, partials);
    lf_sums_finish_kernel<<<1, 64, 0, st>>>(partials, kRedBlocks, out8);
}
void launch_lf_eval(FitDims d, FitWork w, const LfVerts &v, hipStream_t st) { lf_eval_kernel<<<kRedBlocks, 256, 0, st>>>(d, w, v); }

// 40-bin histogram of the log dispersion residuals inside (-10, 10) (hist(breaks = -20:20/2) as hist.default counts
// it, pmc_bin): input of the simulation-matched prior variance for residual d.f. <= 3 (prior_mc.h).  Counts as
// doubles: a sum-all-reducible statistic like the others.
__global__ __launch_bounds__(256) void resid_hist_kernel(FitDims d, FitWork w, double *out) {
    __shared__ unsigned int h[kPmcBins];
    if (threadIdx.x < kPmcBins) h[threadIdx.x] = 0;
    __syncthreads();
    for (int64_t i = blockIdx.x * 256 + threadIdx.x; i < d.n; i += (int64_t)gridDim.x * 256) {
        const int b = pmc_bin(w.resid[i]);  // NaN = not part of the fit
        if (b >= 0) atomicAdd(&h[b], 1u);
    }
    __syncthreads();
    if (threadIdx.x < kPmcBins && h[threadIdx.x]) atomicAdd(&out[threadIdx.x], (double)h[threadIdx.x]);
}
void launch_resid_hist(FitDims d, FitWork w, double *out40, hipStream_t st) {
    (void)hipMemsetAsync(out40, 0, sizeof(double) * 40, st);
    resid_hist_kernel<<<256, 256, 0, st>>>(d, w, out40);
}

// estimateDispersionsPriorVar for residual d.f. <= 3 (prior_mc.h): KL of the observed residual density against the 200
// simulated ones, loess as R evaluates it (local fits at the k-d tree vertices, cubic Hermite in between) on the fine
// grid, first minimum — the pieces of pmc_prior_var(), one workgroup, no host round trip.  t: the table of this
// d.f. (built once per process on the host).
__global__ __launch_bounds__(256) void prior_mc_kernel(FitDims d, FitWork w, const double *hist, const PmcTable *t) {
    __shared__ double obs[kPmcBins], kl[kPmcGrid], s_nobs, bestv[256], vert[kPmcMaxVert], val[kPmcMaxVert], slope[kPmcMaxVert];
    __shared__ int besti[256];
    if (threadIdx.x == 0) {
        double nobs = 0;
        for (int b = 0; b < kPmcBins; b++) nobs += hist[b];
        s_nobs = nobs;
    }
    __syncthreads();
    if (!(s_nobs > 0)) {  // no residuals at all: the closed form (its 0.25 floor)
        if (threadIdx.x == 0) prior_var(w.sc, d.S, d.p, NAN);
        return;
    }
    if (threadIdx.x < kPmcBins) obs[threadIdx.x] = hist[threadIdx.x] / (s_nobs * 0.5);
    __syncthreads();
    for (int g = threadIdx.x; g < kPmcGrid; g += 256) kl[g] = pmc_kl(obs, t->dens[g]);
    __syncthreads();
    const int nvert = t->nvert;
    if ((int)threadIdx.x < nvert) {
        vert[threadIdx.x] = t->vert[threadIdx.x];
        pmc_vertex(*t, threadIdx.x, kl, val[threadIdx.x], slope[threadIdx.x]);
    }
    __syncthreads();
    double best = INFINITY;
    int bi = kPmcFine;
    for (int f = threadIdx.x; f < kPmcFine; f += 256) {
        const double fit = pmc_loess_eval(vert, nvert, val, slope, pmc_fine_x(f));
        if (fit < best) { best = fit; bi = f; }
    }
    bestv[threadIdx.x] = best;
    besti[threadIdx.x] = bi;
    __syncthreads();
    for (int off = 128; off > 0; off >>= 1) {  // which.min: the first minimum
        if ((int)threadIdx.x < off) {
            const double ov = bestv[threadIdx.x + off];
            const int oi = besti[threadIdx.x + off];
            if (ov < bestv[threadIdx.x] || (ov == bestv[threadIdx.x] && oi < besti[threadIdx.x])) {
                bestv[threadIdx.x] = ov;
                besti[threadIdx.x] = oi;
            }
        }
        __syncthreads();
    }
    if (threadIdx.x == 0) {
        const double arg = besti[0] < kPmcFine ? pmc_fine_x(besti[0]) : 0.0;
        prior_var(w.sc, d.S, d.p, arg > 0.25 ? arg : 0.25);
    }
}
void launch_prior_mc(FitDims d, FitWork w, const double *hist40, const void *table, hipStream_t st) {
    prior_mc_kernel<<<1, 256, 0, st>>>(d, w, hist40, (const PmcTable *)table);
}

// estimateDispersionsPriorVar, closed-form branch (A4): fit_state.h
__global__ void prior_var_kernel(FitDims d, FitWork w, double prior_in) { prior_var(w.sc, d.S, d.p, prior_in); }
void launch_prior_var(FitDims d, FitWork w, Opts o, hipStream_t st) {
    prior_var_kernel<<<1, 1, 0, st>>>(d, w, o.dispPriorVarIn);
}

}  // namespace cd
