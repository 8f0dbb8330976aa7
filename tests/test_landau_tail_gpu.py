"""landau_tail on the device (chicdiff_hip_selftest_landau_dev: the function as the "hmp" overlap kernel calls it) at the golden
abscissae of tests/golden/landau_tail.json.  The bound is hmp_twin.LANDAU_BOUND_UNITS — twice the figure the numpy TWIN measures on
the CPU, rounded up to a whole unit, in the units of test_landau_tail.py.  It is not derived from the device's own figure: the
factor two allows for the fused multiply-adds and the device's logarithm.  A device beyond it is a finding about the kernel."""
import math
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import hmp_twin as ht  # noqa: E402


@pytest.fixture(scope="module")
def ctx():
    import __graft_entry__ as g
    g.build()
    from chicdiff_amd import hip
    c = hip.HipContext(0)
    yield c
    c.close()


def on_device(ctx, z):
    t = ctx.torch.from_numpy(np.ascontiguousarray(z, dtype=np.float64)).to(ctx.device)
    return ctx.selftest_landau(t).cpu().numpy()


@pytest.mark.gpu
def test_device_against_golden(ctx):
    g, z = ht.golden()
    got = on_device(ctx, z)
    err = ht.error_units(z, got, g)
    k = int(np.argmax(err))
    print(f"device: off by at most {err[k]:.3f} units, at z = {z[k]!r} (bound {ht.LANDAU_BOUND_UNITS})")
    ht.record("device", float(err[k]), z[k])
    assert err[k] <= ht.LANDAU_BOUND_UNITS, (float(err[k]), z[k])
    assert got[z <= -14.0].tolist() == [1.0] * int((z <= -14.0).sum()) and got[z == math.inf].tolist() == [0.0]
    assert (np.diff(got[np.argsort(z)]) <= 0).all()                                   # non-increasing, the seams' neighbours included


@pytest.mark.gpu
def test_device_range_seams_and_special_values(ctx):
    rng = np.random.default_rng(19)
    z = np.concatenate([rng.uniform(-14, 140, 20000), np.exp(rng.uniform(0, 709, 5000)), -np.exp(rng.uniform(-40, 3, 2000)),
                        [-math.inf, -1e300, -14.0, -3.5, math.inf]])
    got = on_device(ctx, z)
    assert (got <= 1.0).all() and (got >= 0.0).all() and (got[-5:] == [1.0, 1.0, 1.0, 1.0, 0.0]).all()
    twin = ht.landau_tail_twin(z)
    exact = (twin == 0.0) | (twin == 1.0)
    assert np.array_equal(got[exact], twin[exact])
    assert np.isnan(on_device(ctx, np.array([math.nan]))[0])
    for b in ht.table_bounds(ht.load_table()):
        lo, at, hi = on_device(ctx, np.array([math.nextafter(b, -math.inf), b, math.nextafter(b, math.inf)]))
        assert lo >= at >= hi, b
