// objective_probe.hip — the dispersion objective on its own (tests/test_gpu_objective.py): a test entry point, no part of a fit.
#include "disp_objective.h"

namespace cd {

// ---- the objective on its own (tests/test_gpu_objective.py) -------------------------------------------------------------------------
// Every search of disp_kernels.hip stops on what eval_point() / eval_point_spread() return; this kernel returns those values themselves, for points
// the caller chooses: a row's record as prep wrote it -> load_row_mu() -> K evaluations, row per lane, or — live_rows > 0 — with that many
// rows per wave on scattered lanes in the samples-across-lanes layout.  Which layout that is follows disp_fit_kernel's rule for its
// default option (line_search_spread = 1), restated in probe_spread_lg() because the kernel's own lines cannot be shared without
// changing its code (a helper called from there moves its registers and schedule): at most the first power of two >= S lanes per row (two at least), halved at most twice and never below two, the
// most that still holds every live row.  Nothing else of the evaluation is restated: the probe calls the search's functions.
__host__ __device__ inline int probe_spread_lg(int S, int nact) {
    int spread_lg = 1;
    while ((1 << spread_lg) < S) spread_lg++;
    const int lg_min = spread_lg - 2 > 1 ? spread_lg - 2 : 1;
    int lg_t = spread_lg;
    while (lg_t >= lg_min && (nact << lg_t) > 64) lg_t--;
    return lg_t < lg_min ? -1 : lg_t;
}
struct ProbeArgs {
    FitDims d;
    FitWork w;
    Opts o;
    ObjectiveProbe pb;
};
template <bool MAP>
__global__ __launch_bounds__(64) void objective_probe_kernel(ProbeArgs A) {
    extern __shared__ double smem[];
    __shared__ LogEntry s_logtab[64];
    __shared__ ExpEntry s_exptab[64];
    exp_table_to_lds(s_exptab);
    log_table_to_lds(s_logtab);
    const int lane = threadIdx.x;
    const int S = A.d.S, K = A.pb.K;
    const int64_t n = A.d.n;
    double *s_tab = smem;  // one wave: the line search's areas (disp_lds_per_wave)
    double *s_nf = s_tab + kTabSlots * 64;
    int *s_y = reinterpret_cast<int *>(s_nf + S * 64);
    const uint64_t gmask = A.d.gmask;
    const bool p2 = A.d.p == 2;
    const bool spread = A.pb.live_rows > 0;
    const int live = spread ? A.pb.live_rows : 64;
    // row-per-lane: lane l holds the wave's l-th row; samples across lanes: the wave's i-th row sits in lane (37 i + 3) mod 64
    const int slot = spread ? ((lane - 3) * 45) & 63 : lane;  // (45 = 1 / 37 mod 64)
    const int64_t r = (int64_t)blockIdx.x * live + slot;
    bool active = slot < live && r < n;
    if (active) active = load_row_mu(A.w.rowpack + r * row_stride(S), S, s_nf, s_y, lane, gmask, A.o.minmu);  // (an all-zero row has no objective: the searches skip it)
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
    if (slot < live && r < n)
        for (int j = 0; j < S; j++) A.pb.mu[(int64_t)j * n + r] = active ? s_nf[j * 64 + lane] : NAN;
    const double prior_mean = (MAP && active) ? A.pb.prior_mean[r] : 0.0;
    const unsigned long long actmask = __ballot(active);
    const int lg_t = spread ? probe_spread_lg(S, __popcll(actmask)) : -1;
    SpreadMap map = SpreadMap();
    if (spread && lg_t >= 0) map = spread_map(s_tab, lane, lg_t, actmask, active, MAP, prior_mean);
    for (int k = 0; k < K; k++) {
        const double a_eval = active ? A.pb.a[r * K + k] : 0.0;
        double lp = NAN, dlp = NAN, alpha = NAN;
        DIAG(unsigned long long tms[7];)
        if (spread) {
            if (lg_t >= 0) eval_point_spread(s_nf, s_y, s_tab, lane, S, map, gmask, p2, a_eval, MAP, A.pb.prior_isig, lp, dlp, alpha, s_logtab, s_exptab DIAG(, tms));
        } else if (active) {
            eval_point(s_nf, s_y, s_tab, lane, lane, S, gmask, p2, a_eval, MAP, prior_mean, A.pb.prior_isig, lp, dlp, alpha, s_logtab, s_exptab DIAG(, tms));
        }
        if (slot < live && r < n) {
            A.pb.lp[r * K + k] = active ? lp : NAN;
            A.pb.dlp[r * K + k] = active ? dlp : NAN;
            A.pb.alpha[r * K + k] = active ? alpha : NAN;
        }
    }
}
int launch_objective_probe(FitDims d, FitWork w, Opts o, const ObjectiveProbe &pb, hipStream_t st) {
    const int live = pb.live_rows > 0 ? pb.live_rows : 64;
    // (a wave of the probe may hold fewer live rows than asked for — its last, or one with all-zero rows — and takes the layout for
    // those; what is returned is the layout of a full wave)
    const int lg = pb.live_rows > 0 ? probe_spread_lg(d.S, live) : 0;
    if (lg < 0 || live > 64) return -1;
    const ProbeArgs A{d, w, o, pb};
    const unsigned blocks = (unsigned)((d.n + live - 1) / live);
    if (pb.prior_mean) objective_probe_kernel<true><<<blocks, 64, disp_lds_per_wave(d.S), st>>>(A);
    else objective_probe_kernel<false><<<blocks, 64, disp_lds_per_wave(d.S), st>>>(A);
    return 1 << lg;
}

}  // namespace cd
