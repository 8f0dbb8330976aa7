// trend_mad_harness.cpp — TEST-ONLY CPU twins of the persistent trend kernel's two round-saving devices, over the product's own
// state machine and helpers (chicdiff_amd/csrc/fit_state.h):
//   * the trend's pass loop with and without speculative passes (trend_step_spec), over rows or over a script of sums;
//   * the value-binned median / MAD (vb_pick, vb_bracket, vb_check) with the kernel's fallback decisions.
// tests/test_trend_mad_state.py builds and drives it.  It is not part of the product and is never loaded by chicdiff_amd.
#include <math.h>
#include <stdint.h>
#include <string.h>

#include <algorithm>
#include <vector>

#include "../../chicdiff_amd/csrc/fit_state.h"

using namespace cd;

// out: coefs[0], coefs[1], outer_it, conv, failed (2 if the pass budget ran out, as the kernel reports it), passes run,
// speculative sets consumed, passes that speculated
static void report(const FitScalars &sc, int passes, int used, int flagged, double *out) {
    out[0] = sc.coefs[0];
    out[1] = sc.coefs[1];
    out[2] = sc.outer_it;
    out[3] = sc.conv;
    out[4] = sc.finished ? sc.failed : 2;
    out[5] = passes;
    out[6] = used;
    out[7] = flagged;
}
constexpr int kPassBudget = 11 * 27 + 16;  // the kernel's

extern "C" {

// The kernel's pass loop over rows, one workgroup's worth of arithmetic: plain sums in row order.
void harness_trend_rows(const double *baseMean, const double *dispGene, const int32_t *allZero, int64_t n, double minDisp, int32_t speculate,
                        double *out) {
    FitScalars sc;
    memset(&sc, 0, sizeof sc);
    trend_init(&sc);
    int passes = 0, used = 0, flagged = 0;
    for (; passes < kPassBudget && !sc.finished; passes++) {
        const bool spec = sc.spec_next != 0;
        double v[kTrendSums] = {0, 0, 0, 0, 0, 0, 0, 0}, u[kTrendSums] = {0, 0, 0, 0, 0, 0, 0, 0};
        for (int64_t i = 0; i < n; i++) {
            if (allZero[i] || !(dispGene[i] > 100 * minDisp)) continue;
            if (spec) trend_row_spec(&sc, baseMean[i], dispGene[i], v, u);
            else trend_row(&sc, baseMean[i], dispGene[i], v);
        }
        flagged += spec;
        used += trend_step_spec(&sc, v, spec ? u : nullptr, speculate != 0) ? 1 : 0;
    }
    report(sc, passes, used, flagged, out);
}

// The same loop over a script: script[i] holds the sums of the i-th pass of the machine that never speculates.  A speculative
// pass that converges is followed, in that machine, by the start pass of the next glm() call — so its second set of sums is
// script[i + 1], and consuming it skips that entry.
void harness_trend_script(const double *script, int32_t nscript, int32_t speculate, double *out) {
    FitScalars sc;
    memset(&sc, 0, sizeof sc);
    trend_init(&sc);
    int passes = 0, used = 0, flagged = 0;
    const double zero[kTrendSums] = {0, 0, 0, 0, 0, 0, 0, 0};
    for (int i = 0; i < nscript && !sc.finished; passes++) {
        const bool spec = sc.spec_next != 0;
        const double *v = script + (size_t)i * kTrendSums, *u = i + 1 < nscript ? v + kTrendSums : zero;
        flagged += spec;
        const bool took = trend_step_spec(&sc, v, spec ? u : nullptr, speculate != 0);
        used += took;
        i += took ? 2 : 1;
    }
    report(sc, passes, used, flagged, out);
}

// Median and MAD of x[0, n) (NaN = no residual) by the kernel's value-binned route, every step through fit_state.h's helpers;
// where the kernel would turn to its radix select, the order statistics come from a sort of the keys (which is what that select
// computes) and the turn is reported.  cap: keys a candidate list may hold; list2: keys a narrowed list may hold; sort_max: list
// length up to which no narrowing happens (the kernel's kVbCap / kVbList2 / kMadSortMax unless a test says otherwise).
// out: med, mad, population, fallback of the median (0 none, 1 list too long, 2 ties inside the list), fallback of the MAD
// (0 none, 1 check failed, 2 ties inside the list), candidates of the median, candidates of the MAD, rows below the bracket
static bool list_select(std::vector<uint64_t> lst, double vlo, double scale, uint32_t kA, uint32_t kB, int list2, int sort_max, uint64_t *res) {
    if ((int)lst.size() > sort_max) {
        std::vector<uint32_t> cum(kVbSub, 0u);
        for (uint64_t k : lst) cum[(size_t)vb_sub(value_of(k), vlo, scale)]++;
        for (int b = 1; b < kVbSub; b++) cum[(size_t)b] += cum[(size_t)b - 1];
        const int sA = cum_locate(cum.data(), kVbSub, kA), sB = cum_locate(cum.data(), kVbSub, kB);
        const uint32_t below = cum_range(cum.data(), 0, sA - 1), m2 = cum_range(cum.data(), sA, sB);
        if ((int)m2 > list2) return false;
        std::vector<uint64_t> l2;
        for (uint64_t k : lst) {
            const int sb = vb_sub(value_of(k), vlo, scale);
            if (sb == sA || sb == sB) l2.push_back(k);
        }
        if (l2.size() != m2) return false;
        lst.swap(l2);
        kA -= below;
        kB -= below;
    }
    std::sort(lst.begin(), lst.end());
    res[0] = lst[kA];
    res[1] = lst[kB];
    return true;
}
static void sorted_middles(std::vector<uint64_t> keys, uint64_t *res) {
    std::sort(keys.begin(), keys.end());
    res[0] = keys[(keys.size() - 1) / 2];
    res[1] = keys[keys.size() / 2];
}

void harness_value_mad(const double *x, int64_t n, int32_t cap, int32_t list2, int32_t sort_max, double *out) {
    std::vector<uint32_t> cum(kVbBins, 0u);
    for (int64_t i = 0; i < n; i++)
        if (x[i] == x[i]) cum[(size_t)vb_bin(x[i])]++;
    for (int b = 1; b < kVbBins; b++) cum[(size_t)b] += cum[(size_t)b - 1];
    const VbPick pk = vb_pick(cum.data(), kVbBins);
    for (int k = 0; k < 8; k++) out[k] = 0;
    out[0] = out[1] = NAN;
    if (pk.pop == 0) return;
    out[2] = pk.pop;
    out[5] = pk.count;
    uint64_t res[2];
    bool done = false;
    if (pk.count <= (uint32_t)cap) {
        std::vector<uint64_t> lst;
        for (int64_t i = 0; i < n; i++) {
            if (x[i] != x[i]) continue;
            const int b = vb_bin(x[i]);
            if (b == pk.binA || b == pk.binB) lst.push_back(key_of(x[i]));
        }
        const double vlo = (double)pk.binA / kVbScale - kVbOffset, scale = (double)kVbSub * kVbScale / (double)(pk.binB + 1 - pk.binA);
        done = lst.size() == pk.count && list_select(lst, vlo, scale, pk.rankA - pk.below, pk.rankB - pk.below, list2, sort_max, res);
        if (!done) out[3] = 2;
    } else
        out[3] = 1;
    if (!done) {
        std::vector<uint64_t> keys;
        for (int64_t i = 0; i < n; i++)
            if (x[i] == x[i]) keys.push_back(key_of(x[i]));
        sorted_middles(keys, res);
    }
    const double med = (value_of(res[0]) + value_of(res[1])) / 2.0;
    out[0] = med;
    double lo, hi;
    vb_bracket(cum.data(), med, pk.rankA, pk.rankB, &lo, &hi);
    uint32_t pop = 0, below = 0;
    std::vector<uint64_t> lst, all;
    for (int64_t i = 0; i < n; i++) {
        if (x[i] != x[i]) continue;
        const double a = fabs(x[i] - med);
        if (a != a) continue;
        pop++;
        all.push_back(key_of(a));
        if (a < lo) below++;
        else if (a < hi) lst.push_back(key_of(a));
    }
    out[6] = (double)lst.size();
    out[7] = below;
    done = false;
    uint32_t kA = 0, kB = 0;
    if (vb_check(pop, below, (uint32_t)lst.size(), (uint32_t)cap, &kA, &kB)) {
        done = list_select(lst, lo, (double)kVbSub / (hi - lo), kA, kB, list2, sort_max, res);
        if (!done) out[4] = 2;
    } else
        out[4] = 1;
    if (!done) {
        if (all.empty()) {
            out[1] = 1.4826 * NAN;
            return;
        }
        sorted_middles(all, res);
    }
    out[1] = 1.4826 * ((value_of(res[0]) + value_of(res[1])) / 2.0);
}
}
