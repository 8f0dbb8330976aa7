"""Small inputs that reach every path of the dispersion stage (tests/test_disp_twin.py, tests/test_gpu_disp.py).

The designs of tests/wald_inputs.py, 599 rows each: two full 256-thread blocks and a partial wave.  Rows come from synth.make; the fit
runs with trendCoef = (0.05, 2.0) and dispPriorVar = 1.0 given, so a row's two searches depend on the row alone — but for xi (the
column means of nf over the rows that are not all zero) and varLogDispEsts, which the twin forms from the case.

synth.make's own rows already bring, in every design: gene-wise searches of 30-99 steps and of 100 (-> fitDispGrid), no-increase rows
that keep alpha_init, estimates on both sides of the outlier threshold and of alpha_gene > 0.1 alpha_fit, and starts from the rough as
well as from the moments estimate.  Planted beside them (row positions in `case["planted"]`):
  pois    counts = rint(m nf), m = 3 .. 3000: less than Poisson variance.  alpha_init = 1e-8; the first step dives below log(minDisp / 10):
          iter == 1 (not converged under DESeq2's rule), no increase (the row keeps alpha_init), estimate 1e-8;
  giant   counts = rint(c nf) with c up to 1.5e9: the same; from S = 26 on with a first proposal below -30, clamped there (dlp of such
          a row tends to -(S - p) / 2 as mu alpha grows and never passes it, and the clamp needs dlp < -11.6 at the start 1e-8).  Their
          T_lp is 1e10 and more, so dispTol = 1e-6 lies BELOW the rounding of the objective: the MAP search of such a row has no step
          count that double arithmetic could reproduce (the judge's class "below rounding");
  blow    offsets near 2^15 and counts of 0 or 1.8 nf: every q is below 2, so the rough estimate (its mu floored at 1) is 0 and the
          search starts at 1e-8 on a row that is wildly over-dispersed and ends above 1 (not in the interleaved design, where
          the alternating pattern is the group mask itself); in every design some row's proposal lies beyond 10 and is clamped there
          (these, the spike rows or the bulk's: counted over the case);
  huge    one count of 2000 * 2^k, k = 0 .. 10;
  spike   one count alone in a row of zeros: the estimate runs to the ceiling max(10, S), at S = 47 and 64 too;
  wide    offsets spread log-uniformly over 0.05 .. 20 and group means of 0.3 .. 3: some mu_hat sit at the 0.5 floor and some do not;
  zero    three all-zero rows;
  copies  eight of the rows above again at the first, at a middle and at the last row positions.

No row reaches 100 steps in the MAP search at these settings, and none was found that does: with a prior of variance 1 the posterior's
curvature in log alpha is 1 or more, and what lengthens the search — rejections that halve kappa down to the reciprocal of the
curvature — is bounded by log2 of a curvature that int32 counts keep below 2^40 (the longest found: 39 steps).  The prior-aware grid is
reached through the fit's own `maxit` instead: the last case repeats the 4 v 4 design with maxit = 9, where rows of 9 steps or more
go to the grid in both stages.
"""
import numpy as np

import wald_inputs as wi

from chicdiff_amd import synth

N = 599
SEED = 2700
OPTS = dict(trendCoef=(0.05, 2.0), dispPriorVar=1.0)
N_POIS, N_GIANT, N_BLOW, N_HUGE, N_SPIKE, N_WIDE = 12, 4, 4, 11, 8, 24
MAXIT_CASE = "S8-4v4-maxit9"

DESIGNS = dict(wi.DESIGNS)
DESIGNS[MAXIT_CASE] = (8, "halves", "maxit = 9: the grid after both searches, with and without prior")
_cache = {}


def make_case(name):
    if name in _cache:
        return _cache[name]
    S, spec, what = DESIGNS[name]
    group = wi._group(spec, S)
    d = synth.make(N, S)
    counts, nf = d["counts"].astype(np.int64), d["nf"].copy()
    rng = np.random.default_rng(SEED + S)
    A, B = np.flatnonzero(group == 0), np.flatnonzero(group == 1)
    planted = {}
    pos = 8

    def take(key, k):
        nonlocal pos
        planted[key] = np.arange(pos, pos + k)
        pos += k
        return planted[key]

    for t, i in enumerate(take("pois", N_POIS)):
        m = 3.0 * 10 ** (t % 4) * (1 + t // 4)
        counts[i] = np.maximum(np.rint(m * nf[i]), 1)
    for t, i in enumerate(take("giant", N_GIANT)):
        c = min(1.5e9 / nf[i].max(), 1.2e10 / S) / 2 ** t
        counts[i] = np.rint(c * nf[i])
    for t, i in enumerate(take("blow", N_BLOW)):
        nf[i] = 2.0 ** 15 * np.exp(rng.normal(0.0, 0.1, S))
        counts[i] = np.where((np.arange(S) + t) % 2 == 0, np.rint((1.8 - 0.2 * t) * nf[i]), 0)
    for t, i in enumerate(take("huge", N_HUGE)):
        counts[i, 0] = max(counts[i, 0], 1)
        counts[i, rng.integers(0, S)] = 2000 * 2 ** t
    for t, i in enumerate(take("spike", N_SPIKE)):
        counts[i] = 0
        counts[i, (3 * t) % S] = 40 * (t + 1) ** 2
    for t, i in enumerate(take("wide", N_WIDE)):
        nf[i] = np.exp(rng.uniform(np.log(0.05), np.log(20.0), S))
        gm = np.where(group == 1, 0.3 + 0.1 * t, 3.0 - 0.1 * t)
        counts[i] = rng.poisson(gm * nf[i])
        counts[i, A[t % len(A)]] = max(counts[i, A[t % len(A)]], 1)
    counts[take("zero", 3)] = 0
    hard = np.concatenate([planted[k][:n] for k, n in (("pois", 1), ("giant", 1), ("blow", 1), ("huge", 2), ("spike", 1), ("wide", 2))])
    copies = [np.arange(0, 8), np.arange(N // 2 - 4, N // 2 + 4), np.arange(N - 8, N)]
    for dst in copies:
        counts[dst], nf[dst] = counts[hard], nf[hard]
    planted["hard"] = hard
    planted["copies"] = np.stack(copies)  # copies[k, t] is a copy of hard[t]
    assert pos <= N // 2 - 4 and counts.max() <= 2 ** 31 - 1 and counts.min() >= 0
    opts = dict(OPTS)
    if name == MAXIT_CASE:
        opts["maxit"] = 9
    case = dict(name=name, S=S, group=group, counts=np.ascontiguousarray(counts, dtype=np.int32), nf=np.ascontiguousarray(nf), planted=planted,
                what=what, two_groups=bool(len(B)), opts=opts, maxit=opts.get("maxit", 100))
    _cache[name] = case
    return case


# the free fits of the global stage: sizes at which a parametric trend is fitted (tests/test_trend_mad_rounds_gpu.py)
FREE_FITS = {"1500x4": (1500, 4), "2051x8": (2051, 8), "1500x16": (1500, 16)}


def make_free(name):
    n, S = FREE_FITS[name]
    d = synth.make(n, S)
    return dict(name=name, S=S, group=d["group"], counts=np.ascontiguousarray(d["counts"], dtype=np.int32), nf=np.ascontiguousarray(d["nf"]))
