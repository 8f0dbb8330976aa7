// selftest_kernels.hip — the device math as the kernels call it, one function per op, for the tests.
#include "common.h"
#include "devmath.h"
#include "prior_mc.h"

namespace cd {

// device-math self test (tests/test_gpu_parity.py::test_device_math): out[i] = f_op(x[i])
__global__ __launch_bounds__(256) void math_selftest_kernel(int op, const double *__restrict__ x, int64_t n,
                                                            double *__restrict__ out) {
    __shared__ LogEntry s_logtab[64];
    __shared__ ExpEntry s_exptab[64];
    exp_table_to_lds(s_exptab);
    log_table_to_lds(s_logtab);
    for (int64_t i = blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256) {
        const double v = x[i];
        double r = NAN, t;
        switch (op) {
            case 0: r = flog(v); break;
            case 1: r = tlog(v, s_logtab); break;
            case 2: r = rcp(v); break;
            case 3: r = lgamma_pos(v); break;
            case 4: lgamma_digamma(v, t, r); break;
            case 5: r = pnorm_two_sided(v); break;
            case 6: r = __builtin_amdgcn_rcp(v); break;  // raw v_rcp_f64 (~25 bits)
            case 7: { double q = __builtin_amdgcn_rcp(v); r = fma(q, fma(-v, q, 1.0), q); } break;  // + 1 Newton step
            case 8: r = texp(v, s_exptab); break;
            case 9: r = as241(v, FlogFn()); break;  // qnorm as the control draws call it (control_kernels.hip)
        }
        out[i] = r;
    }
}
void launch_math_selftest(int op, const double *x, int64_t n, double *out, hipStream_t st) {
    math_selftest_kernel<<<256, 256, 0, st>>>(op, x, n, out);
}

// the building blocks of the objective, of crow and of the reported deviance, each as its callers form it
// (tests/test_gpu_objective.py): out[i] (and out2[i] where an op has two results) = f_op(x[i], y[i]); y is an integer count
__global__ __launch_bounds__(256) void math3_selftest_kernel(int op, const double *__restrict__ x, const double *__restrict__ y, int64_t n,
                                                             const double *__restrict__ logfact, double *__restrict__ out,
                                                             double *__restrict__ out2) {
    __shared__ LogEntry s_logtab[64];
    log_table_to_lds(s_logtab);
    for (int64_t i = blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256) {
        const double v = x[i];
        const int yi = (int)y[i];
        double r = NAN, r2 = NAN;
        switch (op) {
            case 10: r = lgr_eval_t(lgr_make_t(v, s_logtab), yi, s_logtab); break;
            case 11: r = lgr_eval(lgr_make(v), yi); break;
            case 12: r = lgr_eval(lgr_one(), yi); break;
            case 13: { const double t = 1.0 + v; r = tlog1p_from(v, t, rcp(t), s_logtab); } break;
            case 14: { const double t = 1.0 + v; r = flog1p_from(v, t, rcp(t)); } break;
            case 15: r = rcp_or_div(v); break;
            case 16: stirling(v, tlog(v, s_logtab), rcp(v), r, r2); break;
            case 17: r = rlog_t(v, s_logtab); break;
            case 18: r = (yi >= 0 && yi < kLogFactN) ? logfact[yi] : NAN; break;  // the host's table of log(k!)
        }
        out[i] = r;
        out2[i] = r2;
    }
}
void launch_math3_selftest(int op, const double *x, const double *y, int64_t n, const double *logfact, double *out, double *out2, hipStream_t st) {
    math3_selftest_kernel<<<256, 256, 0, st>>>(op, x, y, n, logfact, out, out2);
}

}  // namespace cd
