"""The persistent trend + MAD kernel with fewer grid-wide rounds: speculative start passes (option "trend_speculate") and the
value-binned median / MAD (option "mad_select_route", three barriers instead of six).  Neither may change a bit: every case is
fitted once per (trend_speculate, mad_select_route) in {0, 1}^2 — (0, 0) runs every pass and the two radix selects — and every
per-row output, the trend coefficients, varLogDispEsts, dispPriorVar, trendOuterIter and status must be identical.
(The decisions of both devices — which passes speculate, when a select turns to the radix rounds — are checked on the CPU, on
the same fit_state.h functions: tests/test_trend_mad_state.py.)"""
import numpy as np
import pytest

from chicdiff_amd import synth

pytestmark = pytest.mark.gpu

COMBOS = [(0, 0), (1, 0), (0, 1), (1, 1)]
TRENDFAILED, PRIORVAR_MC, TREND_LOCAL = 1, 2, 16


@pytest.fixture(scope="module")
def ctx():
    import __graft_entry__ as g
    g.build()  # no-op when the in-tree library and the oracle are up to date
    from chicdiff_amd import hip
    c = hip.HipContext(0)
    yield c
    c.close()


def tied_rows(n):
    """three row patterns repeated: three distinct residuals, a third of the rows each — no candidate list holds a bin"""
    pat = np.array([[2, 9, 1, 12], [40, 70, 35, 90], [400, 520, 380, 610]], np.int32)
    return dict(counts=np.ascontiguousarray(pat[np.arange(n) % 3]), nf=np.ones((n, 4)), group=synth.groups(4))


CASES = {
    # name: (data, options besides the two under test, status bits expected)
    "one_workgroup_1500x4": (lambda: synth.make(1500, 4), {}, PRIORVAR_MC),
    "two_workgroups_2051x4": (lambda: synth.make(2051, 4), {}, PRIORVAR_MC),          # prior variance by simulation, d.f. 2
    "closed_form_prior_30000x8": (lambda: synth.make(30000, 8), {}, 0),
    "rows_beyond_the_lds_cache_70000x8": (lambda: synth.make(70000, 8), {"trend_persistent_blocks": 2}, 0),  # 35 000 rows per workgroup, 8 000 cached
    "value_cap_8_2051x4": (lambda: synth.make(2051, 4), {"mad_value_cap": 8}, PRIORVAR_MC),
    "value_cap_1_2051x4": (lambda: synth.make(2051, 4), {"mad_value_cap": 1}, PRIORVAR_MC),  # (a bin of 2 051 rows holds two or three: 8 does not always force the radix select)
    "massive_ties_20000x4": (lambda: tied_rows(20000), {}, PRIORVAR_MC),
}


@pytest.mark.parametrize("name", list(CASES))
def test_same_bits_for_every_route(ctx, name):
    from chicdiff_amd import hip
    make, extra, status_bits = CASES[name]
    d = make()
    dk = ctx.to_device(d["counts"], np.int32)
    dn = ctx.to_device(d["nf"], np.float64)
    want = hip.OUT_DOUBLE + hip.OUT_INT
    runs = {}
    try:
        for k, v in extra.items():
            ctx.set_option(k, v)
        for spec, route in COMBOS:
            ctx.set_option("trend_speculate", spec)
            ctx.set_option("mad_select_route", route)
            out, sc = ctx.nbglm_fit(dk, dn, d["group"], want=want)
            runs[(spec, route)] = ({k: out[k].cpu().numpy().copy() for k in want}, sc)
    finally:
        ctx.set_option("trend_speculate", 1)
        ctx.set_option("mad_select_route", 1)
        for k in extra:
            ctx.set_option(k, 0)
    ref_out, ref_sc = runs[(0, 0)]
    print(name, ref_sc)
    assert (ref_sc["status"] & (TRENDFAILED | TREND_LOCAL)) == 0 and (ref_sc["status"] & PRIORVAR_MC) == status_bits  # the parametric trend, from this kernel
    assert np.isfinite(ref_sc["varLogDispEsts"]) and ref_sc["trendOuterIter"] >= 1
    for combo in COMBOS[1:]:
        out, sc = runs[combo]
        for k in ("trendCoef", "varLogDispEsts", "dispPriorVar", "trendOuterIter", "status", "sumDeviance"):
            assert np.asarray(sc[k], np.float64).tobytes() == np.asarray(ref_sc[k], np.float64).tobytes(), (combo, k, sc[k], ref_sc[k])
        for k in want:
            assert out[k].tobytes() == ref_out[k].tobytes(), (combo, k, int(np.sum(out[k] != ref_out[k])))
