"""Option "wald_final_row_constant": for a row the IRLS converged on, wald_final_kernel takes sum_j y_j log(alpha mu_j) from the row
constant wald_prep left (crow + sum_j y_j (log alpha + log nf_j)) plus eta_A sum_A y + eta_B sum_B y, instead of a logarithm of mu per
sample.  The fits of tests/wald_route_inputs.py with the option on and off: every output array_equal except `deviance` and `sumDeviance`.

deviance:  |new - old| <= 2^-45 (|old| + 2 sum_j y_j |log(alpha mu_j)|) per row, the sum formed here from the fit's own outputs
(dispersion, intercept, log2FoldChange, and the offsets the context forms from its size factors).  Both routes add the same 2 S + O(1)
terms in another association, each rounding is at most 2^-53 of a partial sum, and S <= 64 gives (2 * 64 + 8) 2^-53 < 2^-45.
A row the optim fallback produced keeps the per-sample sum and must be bit-identical; the matrices of 63 rows and more hold such rows
(asserted).  sumDeviance: the same bound summed over the rows.
"""
import numpy as np
import pytest

import wald_route_inputs as wr

LN2 = float(np.log(2.0))


@pytest.fixture(scope="module")
def ctxs():
    import __graft_entry__ as g
    g.build()
    from chicdiff_amd import hip
    on, off = hip.HipContext(0), hip.HipContext(0)
    off.set_option("wald_final_row_constant", 0)
    yield on, off
    on.close()
    off.close()


def test_the_matrices_hold_both_kinds_of_row():
    """on the CPU, with the oracle: rows that end in the optim fallback (the per-sample sum, floored mu) beside converged ones, rows with
    a sample at the minmu floor at the start, all-zero rows"""
    import __graft_entry__ as g
    g.build()
    for name, (nA, nB, n, _, _) in wr.SHAPES.items():
        if n != 4097 or nA + nB == 2:
            continue
        case = wr.make_shape(name)
        o = wr.oracle_view(case)
        ref, p = o["ref"], case["planted"]
        optim = o["live"] & (ref["betaIter"] >= 100)
        print(f"{name}: floored at the start {int(o['floored'].sum())}, all zero {int((~o['live']).sum())}, first solve beyond 30 "
              f"{int(o['beyond30'].sum())}, optim fallback {int(optim.sum())}, longest IRLS short of it {int(ref['betaIter'][o['live'] & ~optim].max())}")
        assert o["floored"].sum() > 0 and (~o["live"]).sum() >= 4 and np.all(~o["live"][p["zero"]])
        assert optim.sum() > 0 and np.all(optim[o["beyond30"]]) and (o["live"] & ~optim).sum() > 4000
        if (nA, nB) == (4, 4):
            assert np.all(o["floored"][p["floor"]]) and np.all(optim[p["huge"]])  # one count of 10^6 among zeros
        assert np.any(ref["betaIter"][p["big"]] >= 10) and np.any(~optim[p["big"]])


@pytest.mark.gpu
@pytest.mark.parametrize("name,spread", wr.CASES, ids=[f"{n}-spread{s}" for n, s in wr.CASES])
def test_row_constant_moves_only_the_deviance_and_within_its_rounding(ctxs, name, spread):
    on, off = ctxs
    case = wr.make_shape(name)
    a, b = wr.fit(on, case, spread), wr.fit(off, case, spread)
    assert a[0] == b[0], (a[:2], b[:2])
    if case["S"] == 2:
        assert a[0] == "error" and a[1] == b[1] and "no residual degrees of freedom" in a[1]
        return
    assert a[0] == "ok", a[1]
    new, old = a[1], b[1]
    for k in wr.ALL_COLUMNS:
        if k != "deviance":
            assert np.array_equal(new[k], old[k], equal_nan=True), k
    wr.same_scalars(a[2], b[2], but=("sumDeviance",))
    live = old["allZero"] == 0
    assert np.array_equal(np.isnan(new["deviance"]), ~live) and np.array_equal(np.isnan(old["deviance"]), ~live)
    # sum_j y_j |log(alpha mu_j)| from the fit's own outputs
    dfm = off.to_device(case["fullmean"], np.float64)
    nf = off.offsets(dfm, b[2]["sizeFactors"], wr.THETA).cpu().numpy().T  # (n, S)
    B = (case["group"] == 1)[None, :]
    with np.errstate(all="ignore"):
        eta = np.where(B, (old["intercept"] + old["log2FoldChange"])[:, None], old["intercept"][:, None]) * LN2
        optim = live & (old["betaIter"] >= 100)
        mu = nf * np.exp(eta)
        mu = np.where(optim[:, None], np.maximum(mu, wr.MINMU), mu)
        y = case["counts"].astype(np.float64)
        terms = np.where(y > 0, y * np.abs(np.log(old["dispersion"][:, None] * mu)), 0.0).sum(1)
    bound = 2.0 ** -45 * (np.abs(old["deviance"]) + 2.0 * terms)
    diff = np.abs(new["deviance"] - old["deviance"])
    assert np.all(np.isfinite(bound[live]))
    worst = np.nanmax(np.where(live, diff / bound, 0.0)) if live.any() else 0.0
    print(f"{name} spread {spread}: deviance differs in {int((diff[live] > 0).sum())} of {int(live.sum())} rows, largest |new - old| / bound "
          f"{worst:.3g}; {int(optim.sum())} rows of the optim fallback")
    assert np.all(diff[live] <= bound[live]), np.flatnonzero(live & ~(diff <= bound))[:10]
    assert np.array_equal(new["deviance"][optim], old["deviance"][optim])
    if case["n"] >= 63:
        assert optim.sum() > 0
    sd_new, sd_old = a[2]["sumDeviance"], b[2]["sumDeviance"]
    print(f"    sumDeviance {sd_new!r} against {sd_old!r}: relative difference {abs(sd_new - sd_old) / abs(sd_old):.3g}")
    if np.isnan(sd_old) or np.isnan(sd_new):  # (a fit with all-zero rows reports NaN, as sum() over R's column with its NA does)
        assert np.isnan(sd_old) and np.isnan(sd_new)
        return
    # the rows' bounds, and the two sums' own roundings (each a tree over at most 2^31 terms: 64 roundings of the total's size at most)
    assert abs(sd_new - sd_old) <= bound[live].sum() + 2.0 ** -46 * np.abs(old["deviance"][live]).sum()
