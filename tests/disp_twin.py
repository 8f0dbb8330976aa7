"""The dispersion stage (estimateDispersionsGeneEst -> estimateDispersionsFit -> estimateDispersionsMAP) in 50-digit arithmetic (mpmath).

Written from SURVEY.md Appendix A1-A4 and the column descriptions of include/chicdiff_hip.h — not from the CPU oracle, not from
tests/np_twin.py and not from the kernels — so that tests/test_disp_twin.py and tests/test_gpu_disp.py can hold either of them to
something that shares no code and no rounding with it.  Three functions:

  closed_forms(counts, nf, group)   per row: allZero, baseMean, baseVar, group means, mu_hat, the rough and the moments estimate (xi
                                    from the column means of nf over the rows that are not all zero) and alpha_init;
  replay(y, mu, group, start, ...)  fitDisp step by step (A2.6-A2.7, A4): every proposal, every decision and its margin, the grid;
  global_stage(...)                 the parametric trend, dispFit, the MAD of the log residuals and the prior variance (A3, A4).

Every value is an mpf of DPS digits; callers work inside `with mp.workdps(DPS)`.  Every value comes with its UNIT: u = 2^-52 times the
sum of the absolute values of the terms it is formed from, before they cancel (the convention of mp_objective in
tests/test_gpu_objective.py); errors of a double-precision fit are counted in these units.
"""
import mpmath as mp

DPS = 50
U = mp.ldexp(mp.mpf(1), -52)

MIN_DISP = 1e-8
DISP_TOL = 1e-6
KAPPA0 = 1.0
EPSILON = 1e-4
N_GRID = 20


def max_disp(S):
    return float(max(10, S))


# ---------------------------------------------------------------------------------------------------------------------------
# A2.1 - A2.5: closed forms of a case
# ---------------------------------------------------------------------------------------------------------------------------
def closed_forms(counts, nf, group):
    """Per row of a whole case (xi needs every column of nf).  Returns a list of dicts, one per row:
    allZero, baseMean, baseVar, gmean (one per sample: the mean of q over the sample's group), mu (max(nf gmean, 0.5)), mufloored (how
    many), rough, moments, init (alpha_init), branch ("rough" / "moments": which of the two is the smaller), clamped (alpha_init sits on
    a bound), and `unit` = {quantity: unit}.  All-zero rows carry allZero only.  `xi` is returned as the second value."""
    n, S = len(counts), len(group)
    g = [int(v != 0) for v in group]
    p = 2 if any(g) else 1
    size = [g.count(0), g.count(1)]
    live = [i for i in range(n) if any(int(v) for v in counts[i])]
    fv = {i: [mp.mpf(float(v)) for v in nf[i]] for i in live}
    xi = mp.fsum(len(live) / mp.fsum(fv[i][j] for i in live) for j in range(S)) / S
    half, one = mp.mpf(0.5), mp.mpf(1)
    lo, hi = mp.mpf(MIN_DISP), mp.mpf(max_disp(S))
    out = []
    for i in range(n):
        if i not in fv:
            out.append(dict(allZero=1))
            continue
        f = fv[i]
        q = [mp.mpf(int(a)) / b for a, b in zip(counts[i], f)]
        bm = mp.fsum(q) / S
        d = [x - bm for x in q]
        bv = mp.fsum(x * x for x in d) / (S - 1)
        # each difference carries u (|q| + |mean|) from its inputs: charged to them, not to whoever squares it
        u_bv = U * (mp.fsum(2 * abs(x) * (abs(a) + bm) for x, a in zip(d, q)) / (S - 1) + bv)
        gm = [mp.fsum(x for x, gj in zip(q, g) if gj == c) / size[c] if size[c] else None for c in (0, 1)]
        gmean = [gm[gj] for gj in g]
        muf = [b * m for b, m in zip(f, gmean)]
        mu = [m if m > half else half for m in muf]
        m1 = [m if m > one else one for m in gmean]  # the rough estimate's own floor: mu_lin at 1
        terms = [((x - m) ** 2 - m) / (m * m) for x, m in zip(q, m1)]
        rough = mp.fsum(terms) / (S - p)
        u_rough = U * mp.fsum((2 * abs(x - m) * (abs(x) + m) + (x - m) ** 2 + m) / (m * m) for x, m in zip(q, m1)) / (S - p)
        if rough < 0:
            rough = mp.mpf(0)
        moments = (bv - xi * bm) / (bm * bm)
        u_mom = (u_bv + U * (bv + 2 * xi * bm)) / (bm * bm) + U * abs(moments)
        branch = "rough" if rough <= moments else "moments"
        a0, u0 = (rough, u_rough) if branch == "rough" else (moments, u_mom)
        clamped = not (lo < a0 < hi)
        init = lo if a0 <= lo else hi if a0 >= hi else a0
        out.append(dict(allZero=0, baseMean=bm, baseVar=bv, gmean=gmean, mu=mu, mufloored=sum(1 for m in muf if m < half), rough=rough,
                        moments=moments, init=init, branch=branch, clamped=clamped, raw_init=a0,
                        unit=dict(baseMean=U * bm, baseVar=u_bv, rough=u_rough, moments=u_mom, init=u0)))
    return out, xi


# ---------------------------------------------------------------------------------------------------------------------------
# A2.6: the objective
# ---------------------------------------------------------------------------------------------------------------------------
class Objective:
    """log posterior of a = log(alpha) for one row (counts y, means mu as given, design by `group`), its derivative, and the sums T of
    the absolute values of their terms before cancellation.  prior = (mean of log alpha, variance) or None.  Values are kept by a."""

    def __init__(self, y, mu, group, prior=None):
        g = [int(v != 0) for v in group]
        self.p2 = any(g)
        self.rows = [(int(a), mp.mpf(m), gj if self.p2 else 0) for a, m, gj in zip(y, mu, g)]
        self.prior = None if prior is None else (mp.mpf(prior[0]), mp.mpf(prior[1]))
        self._lp, self._dlp = {}, {}

    def _cr(self, al, deriv):
        w, dw = [mp.mpf(0), mp.mpf(0)], [mp.mpf(0), mp.mpf(0)]
        for _, m, k in self.rows:
            t = 1 / m + al
            w[k] += 1 / t
            if deriv:
                dw[k] -= 1 / (t * t)
        return w, dw

    def lp(self, a, cox_reid=True):
        """(lp, T_lp) at a."""
        key = (a, cox_reid)
        if key in self._lp:
            return self._lp[key]
        al = mp.exp(a)
        r = 1 / al
        lg_r = mp.loggamma(r)
        lgy = {0: lg_r}
        ll = T = mp.mpf(0)
        for y, m, _ in self.rows:
            if y not in lgy:
                lgy[y] = mp.loggamma(y + r)
            t2, t3 = y * mp.log(m + r), r * mp.log1p(m * al)
            ll += lgy[y] - lg_r - t2 - t3
            T += abs(lgy[y]) + abs(lg_r) + abs(t2) + abs(t3)
        if cox_reid:
            w, _ = self._cr(al, False)
            cr = -mp.log(w[0] * w[1] if self.p2 else w[0]) / 2
            ll, T = ll + cr, T + abs(cr)
        if self.prior is not None:
            pr = -((a - self.prior[0]) ** 2) / (2 * self.prior[1])
            ll, T = ll + pr, T + abs(pr)
        self._lp[key] = (ll, T)
        return ll, T

    def dlp(self, a, cox_reid=True):
        """(dlp, T_dlp) at a."""
        key = (a, cox_reid)
        if key in self._dlp:
            return self._dlp[key]
        al = mp.exp(a)
        r = 1 / al
        dg_r = mp.digamma(r)
        dgy = {0: dg_r}
        s = Ts = mp.mpf(0)
        for y, m, _ in self.rows:
            if y not in dgy:
                dgy[y] = mp.digamma(y + r)
            ma = m * al
            L, q1, q2 = mp.log1p(ma), ma / (1 + ma), y / (m + r)
            s += dg_r + L - q1 - dgy[y] + q2
            Ts += abs(dg_r) + abs(L) + abs(q1) + abs(dgy[y]) + abs(q2)
        d, Td = r * s, r * Ts
        if cox_reid:
            w, dw = self._cr(al, True)
            ks = (0, 1) if self.p2 else (0,)
            d -= al * mp.fsum(dw[k] / w[k] for k in ks) / 2
            Td += al * mp.fsum(abs(dw[k] / w[k]) for k in ks) / 2
        if self.prior is not None:
            dpr = -(a - self.prior[0]) / self.prior[1]
            d, Td = d + dpr, Td + abs(dpr)
        self._dlp[key] = (d, Td)
        return d, Td


# ---------------------------------------------------------------------------------------------------------------------------
# A2.6 - A2.7, A4: the line search and the grid
# ---------------------------------------------------------------------------------------------------------------------------
def replay(y, mu, group, start, prior=None, maxit=100, flip=(), S=None, objective=None):
    """fitDisp from log(start) (`start`: a double, taken as exact) and what follows it.  prior=None: the gene-wise search with its
    cap at maxDisp, the no-increase revert to `start`, conv = iter < maxit and iter != 1, and the grid for rows not converged whose alpha
    is above 1e-7.  prior=(mean of log alpha, variance): the MAP search; the grid (with the prior) for iter >= maxit.  Both end in the
    clamp to [1e-8, max(10, S)].

    Returns dict(alpha, log_alpha (of the search's or the grid's end, before revert and clamp), iter, path = [(step, "accept" | "reject")],
    grid, reverted, clamped ("floor" | "ceiling" | None), proposals_clamped = [(step, 10 | -30)], unit (of the final log alpha:
    u (1 + |a| + sum over accepted steps of kappa_k T_dlp(a_k))), decisions).  A decision is a dict(kind, step, margin, points, T): `margin`
    is the quantity whose sign decides (mpf), `points` the values of a whose objective enters it, `T` = the sum of the T_lp at those
    points (kinds "a-floor", "cap" and "grid-gate" compare a or alpha itself: T is then that value's own unit over u).  `flip`: indices into
    `decisions` that are taken the other way (for rows whose margin lies inside double rounding)."""
    S = len(y) if S is None else S
    obj = objective or Objective(y, mu, group, prior)
    a = mp.log(mp.mpf(float(start)))
    a_start = a
    lo, hi = mp.mpf(-30), mp.mpf(10)
    min_log_alpha = mp.log(mp.mpf(MIN_DISP) / 10)
    eps, tol = mp.mpf(EPSILON), mp.mpf(DISP_TOL)
    kappa = mp.mpf(KAPPA0)
    decisions, path, clampedp = [], [], []

    def decide(kind, step, margin, points, T, strict=True):
        """True when margin > 0 (strict) or >= 0 — or the flipped answer."""
        decisions.append(dict(kind=kind, step=step, margin=margin, points=points, T=T))
        ans = margin > 0 if strict else margin >= 0
        return (not ans) if (len(decisions) - 1) in flip else ans

    lp, T = obj.lp(a)
    dlp, Td = obj.dlp(a)
    lp0, T0 = lp, T
    it = accepts = 0
    drift = mp.mpf(0)  # sum of kappa_k T_dlp(a_k) over accepted steps
    for t in range(maxit):
        it += 1
        prop = a + kappa * dlp
        if prop < lo:
            kappa = (lo - a) / dlp
            clampedp.append((it, -30))
        if prop > hi:
            kappa = (hi - a) / dlp
            clampedp.append((it, 10))
        new = a + kappa * dlp
        lpn, Tn = obj.lp(new)
        # Armijo: -lp(new) <= -lp - kappa eps dlp^2
        if decide("armijo", it, lpn - lp - kappa * eps * dlp * dlp, (a, new), T + Tn, strict=False):
            path.append((it, "accept"))
            accepts += 1
            drift += kappa * Td
            # stop when change < tol
            if not decide("change", it, lpn - lp - tol, (a, new), T + Tn, strict=False):
                a, lp, T = new, lpn, Tn
                break
            a = new
            if decide("a-floor", it, min_log_alpha - a, (a,), abs(a) + drift):
                break  # (lp stays that of the step before: fitDisp leaves the loop before it takes the new one over)
            lp, T = lpn, Tn
            dlp, Td = obj.dlp(a)
            kappa = min(kappa * mp.mpf(1.1), mp.mpf(KAPPA0))
            if accepts % 5 == 0:
                kappa = kappa / 2
        else:
            path.append((it, "reject"))
            kappa = kappa / 2
    unit = U * (1 + abs(a) + drift)  # (1: alpha = exp(a) is itself rounded, which moves log alpha by u / 2 whatever |a| is)
    md = mp.mpf(max_disp(S))
    alpha = mp.exp(a)
    grid, reverted = False, False
    if prior is None:
        if decide("cap", it, alpha - md, (a,), md * (abs(a) + drift)):
            alpha = md
        # no increase: last_lp < initial_lp + |initial_lp| / 1e6
        if decide("revert", it, lp0 + abs(lp0) / mp.mpf(1e6) - lp, (a_start, a), T0 + T):
            alpha, reverted = mp.mpf(float(start)), True
        conv = it < maxit and it != 1
        want_grid = (not conv) and decide("grid-gate", it, alpha - mp.mpf(1e-7), (a,), alpha * (abs(a) + drift))
    else:
        want_grid = it >= maxit
    if want_grid:
        grid = True
        alpha, a = _grid(obj, S, decide)
        a_lo = mp.log(mp.mpf(MIN_DISP))
        unit = U * (1 + 2 * abs(a_lo) + 2 * abs(a - a_lo))  # a grid point is a_lo + k step, twice over (coarse, fine): the terms before they cancel
    clamped = None
    if alpha <= mp.mpf(MIN_DISP):
        alpha, clamped = mp.mpf(MIN_DISP), "floor"
    elif alpha >= md:
        alpha, clamped = md, "ceiling"
    return dict(alpha=alpha, log_alpha=a, iter=it, path=path, grid=grid, reverted=reverted, clamped=clamped, proposals_clamped=clampedp,
                unit=unit, decisions=decisions, accepts=accepts)


def _grid(obj, S, decide):
    """fitDispGrid: 20 points on [log 1e-8, log max(10, S)], then 20 on +- one coarse step around the first maximum; the first maximum
    of the fine grid is the result.  Every other point's distance from the winner is a decision (a point before the winner must be
    strictly smaller, a point after it smaller or equal)."""
    a_lo, a_hi = mp.log(mp.mpf(MIN_DISP)), mp.log(mp.mpf(max_disp(S)))
    pts = [a_lo + (a_hi - a_lo) * k / (N_GRID - 1) for k in range(N_GRID)]
    delta = pts[1] - pts[0]
    best = None
    for stage in ("grid-coarse", "grid-fine"):
        vals = [obj.lp(x) for x in pts]
        w = 0
        for j in range(1, len(pts)):
            if vals[j][0] > vals[w][0]:  # a later point wins only when strictly larger: the first maximum stands
                w = j
        k = w
        for j in range(len(pts)):
            # every other point against the winner; taken the other way, that point wins
            if j != w and not decide(stage, j, vals[w][0] - vals[j][0], (pts[w], pts[j]), vals[j][1] + vals[w][1], strict=j < w):
                k = j
        best = pts[k]
        pts = [best - delta + 2 * delta * j / (N_GRID - 1) for j in range(N_GRID)]
    return mp.exp(best), best


# ---------------------------------------------------------------------------------------------------------------------------
# A3, A4: trend, MAD, prior variance
# ---------------------------------------------------------------------------------------------------------------------------
def _median(v):
    s = sorted(v)
    n = len(s)
    return s[n // 2] if n % 2 else (s[n // 2 - 1] + s[n // 2]) / 2


def _gamma_identity_glm(x, yv, start, eps=mp.mpf(1e-8), maxit=25):
    """R's glm(y ~ x, Gamma(link = "identity"), start): IRLS with weights 1 / mu^2 and working response y.  Returns (coefs, converged,
    condition of the last normal matrix, smallest relative distance of a convergence test from eps)."""
    c0, c1 = start
    dev = lambda c0, c1: 2 * mp.fsum((b - (c0 + c1 * a)) / (c0 + c1 * a) - mp.log(b / (c0 + c1 * a)) for a, b in zip(x, yv))
    devold = dev(c0, c1)
    conv, kappa, closest = False, mp.mpf(1), mp.inf
    for _ in range(maxit):
        w = [1 / (c0 + c1 * a) ** 2 for a in x]
        s0, s1, s2 = mp.fsum(w), mp.fsum(wi * a for wi, a in zip(w, x)), mp.fsum(wi * a * a for wi, a in zip(w, x))
        t0, t1 = mp.fsum(wi * b for wi, b in zip(w, yv)), mp.fsum(wi * a * b for wi, a, b in zip(w, x, yv))
        det = s0 * s2 - s1 * s1
        c0, c1 = (s2 * t0 - s1 * t1) / det, (s0 * t1 - s1 * t0) / det
        kappa = (s0 * s2 + s1 * s1) / det
        if any(c0 + c1 * a <= 0 for a in x):
            raise ArithmeticError("Gamma glm: a fitted mean is not positive (R would halve the step: not restated here)")
        d = dev(c0, c1)
        test = abs(d - devold) / (abs(d) + mp.mpf(0.1))
        closest = min(closest, abs(test / eps - 1))
        devold = d
        if test < eps:
            conv = True
            break
    return (c0, c1), conv, kappa, closest


def mad_stage(x, ux):
    """varLogDispEsts = (1.4826 mad)^2 of the residuals x = {row: value} with units ux = {row: unit}.  Returns (v, median, mad, unit of v).
    The medians are order statistics: their error is that of the elements next to them — bounded here by the largest unit among the
    residuals within one mad-width of the two medians, twice (median and deviation), relative to mad, twice again for the square."""
    keep = list(x)
    med = _median([x[i] for i in keep])
    mad = _median([abs(x[i] - med) for i in keep])
    v = (mp.mpf(1.4826) * mad) ** 2
    near_el = [ux[i] for i in keep if abs(abs(x[i] - med) - mad) <= mad / 8 or abs(x[i] - med) <= mad / 8]
    if mad == 0:  # every residual between the two medians is one value: v = 0, and an error of the elements enters squared
        return v, med, mad, (mp.mpf(1.4826) * 2 * (2 * max(near_el) + U * abs(med))) ** 2
    u_v = 2 * v * (2 * max(near_el) + U * (abs(med) + mad)) / mad + U * v
    return v, med, mad, u_v


def global_stage(baseMean, dispGeneEst, S, p, coefs=None, dens=None):
    """Trend, dispFit, varLogDispEsts and dispPriorVar from the REPORTED baseMean and dispGeneEst (doubles, taken as exact; NaN rows —
    all-zero rows — are left out).  `coefs` given: the trend is not fitted (the pinned cases).  Returns dict(coefs, rounds (glm calls;
    None when the trend failed: a coefficient <= 0 or more than 10 rounds), failed, dispFit (per row given, None for NaN rows),
    varLogDispEsts, dispPriorVar (m - p <= 3: matched by simulation, tests/trend_twin.prior_var_mc on the histogram of the residuals
    and the simulated densities `dens`, by default those of the library's host entry; `prior` then holds that function's result and
    `hist` the counts with each residual's distance from a break), unit = {coefs: (u0, u1), dispFit: [..], varLogDispEsts,
    dispPriorVar (m - p <= 3: one unit of the grid value — the result is a grid point, right or wrong)}, near = the smallest
    relative distance of any filter ratio from 1e-4 / 15, of the outer test from
    1e-6 and of a glm convergence test from 1e-8)."""
    rows = [i for i in range(len(baseMean)) if baseMean[i] == baseMean[i] and dispGeneEst[i] == dispGeneEst[i]]
    bm = {i: mp.mpf(float(baseMean[i])) for i in rows}
    al = {i: mp.mpf(float(dispGeneEst[i])) for i in rows}
    res = dict(failed=False, rounds=None, near=mp.inf)
    kappa = mp.mpf(1)
    if coefs is None:
        use = [i for i in rows if al[i] > mp.mpf(100 * MIN_DISP)]
        c = (mp.mpf(0.1), mp.mpf(1))
        rounds = 0
        r_lo, r_hi = mp.mpf(1e-4), mp.mpf(15)
        while True:
            ratio = {i: al[i] / (c[0] + c[1] / bm[i]) for i in use}
            good = [i for i in use if r_lo < ratio[i] < r_hi]
            res["near"] = min([res["near"]] + [min(abs(ratio[i] / r_lo - 1), abs(ratio[i] / r_hi - 1)) for i in use])
            new, conv, kappa, closest = _gamma_identity_glm([1 / bm[i] for i in good], [al[i] for i in good], c)
            rounds += 1
            res["near"] = min(res["near"], closest)
            old, c = c, new
            if not (c[0] > 0 and c[1] > 0):
                res["failed"] = True
                break
            move = mp.log(c[0] / old[0]) ** 2 + mp.log(c[1] / old[1]) ** 2
            res["near"] = min(res["near"], abs(move / mp.mpf(1e-6) - 1))
            if move < mp.mpf(1e-6) and conv:
                break
            if rounds > 10:
                res["failed"] = True
                break
        res["rounds"] = None if res["failed"] else rounds
    else:
        c = (mp.mpf(float(coefs[0])), mp.mpf(float(coefs[1])))
    res["coefs"] = c
    if res["failed"]:
        return res
    fit = {i: c[0] + c[1] / bm[i] for i in rows}
    res["dispFit"] = [fit.get(i) for i in range(len(baseMean))]
    u_fit = {i: U * (abs(c[0]) + abs(c[1] / bm[i])) for i in rows}
    keep = [i for i in rows if al[i] >= mp.mpf(100 * MIN_DISP)]
    x = {i: mp.log(al[i]) - mp.log(fit[i]) for i in keep}
    ux = {i: U * (abs(mp.log(al[i])) + abs(mp.log(fit[i]))) + u_fit[i] / fit[i] for i in keep}
    v, med, mad, u_v = mad_stage(x, ux)
    res.update(varLogDispEsts=v, residual_median=med, mad=mad)
    m = S - p
    tri = mp.polygamma(1, mp.mpf(m) / 2)
    if m > 3:
        pv = v - tri
        res["dispPriorVar"] = pv if pv > mp.mpf(0.25) else mp.mpf(0.25)
        u_pv = u_v + U * (v + tri)
    else:
        import trend_twin as tt
        n = len(baseMean)
        counts, info = tt.resid_hist([x.get(i) for i in range(n)], [ux.get(i) for i in range(n)])
        pm = tt.prior_var_mc(counts, tt.simulated_densities(m) if dens is None else dens, m, var_log_disp_ests=v)
        res.update(dispPriorVar=pm["value"], prior=pm, hist=(counts, info))
        u_pv = U * pm["value"]
    res["unit"] = dict(coefs=(U * kappa * abs(c[0]), U * kappa * abs(c[1])), dispFit=[u_fit.get(i) for i in range(len(baseMean))], varLogDispEsts=u_v,
                       dispPriorVar=u_pv)
    return res


def outlier_rule(dispGeneEst, dispFit, varLogDispEsts, sd=2.0):
    """(is outlier, margin, magnitude compared) of log alpha_gene > log alpha_fit + sd sqrt(varLogDispEsts) on reported doubles."""
    lg, lf = mp.log(mp.mpf(float(dispGeneEst))), mp.log(mp.mpf(float(dispFit)))
    w = mp.mpf(sd) * mp.sqrt(mp.mpf(float(varLogDispEsts)))
    margin = lg - lf - w
    return margin > 0, margin, abs(lg) + abs(lf) + w


def map_start(dispGeneEst, dispFit):
    """(start, margin, magnitude compared) of alpha_gene > 0.1 alpha_fit ? alpha_gene : alpha_fit on reported doubles."""
    g, f = mp.mpf(float(dispGeneEst)), mp.mpf(float(dispFit))
    margin = g - mp.mpf(0.1) * f
    return (float(dispGeneEst) if margin > 0 else float(dispFit)), margin, g + mp.mpf(0.1) * f
