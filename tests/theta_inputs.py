"""Inputs of tests/test_theta_inputs.py and tests/test_gpu_theta_scan.py: the theta scan (chicdiff_hip_theta_grid_dev) and the trend as
one launch per pass (trend_pass_kernel + trend_reduce_kernel, then resid_kernel, two selects and prior_var_kernel / prior_mc), the
route every fit of a scan with more than one theta in flight takes.  Seeded and small.

A scan case is dict(name, counts (n, S) int32, FullMean (n, S), sf (the oracle's size factors of counts), thetas, planted):
  scan-S4, scan-S8, scan-S17  counts and FullMean as tests/test_gpu_parity.py::test_theta_grid builds them (synth.make(n, S, fragments = 3)
              and oracle.window_sums), n = 1500, 2051, 1500 (the sizes of disp_inputs.FREE_FITS) before the all-zero rows are removed;
              every fit of a scan has design ~1.  S = 4: 3 residual d.f., so prior_mc and its table run inside every lane; S = 17: past the
              16 samples of the offsets formed inside prep, so offsets_kernel runs in the lanes.  Grid: the reference's five points;
  scan-zero   scan-S8 with an all-zero row planted first, in the middle and last (planted["zero"]);
  scan-na     scan-S8 with NaN in FullMean in row 0, in the last row and in the first row of the partial last 256-row tile
              (planted["na"]: (row, sample)), as tests/test_prep_offsets_classes_gpu.py plants them;
  sum-sizes   the first n rows of scan-S8, n = 1, 255, 256, 257, 1025 (dev_sum_kernel is one block of 256 threads), fitted under the pinned
              trend and prior of disp_inputs.OPTS: a handful of rows carries no trend.

A trend-edges case is a stage case of tests/trend_inputs.py (baseMean, dispGeneEst, allZero, S, p, opts: fitType parametric, no trend
supplied) for chicdiff_hip_selftest_global_stage_dev, its columns from trend_inputs._trend_columns, with `planted`:
  trend-edges-599   all-zero rows (NaN in both columns) first, last and in a run of 70 in the middle; rows below, at and just above
              100 minDisp among them; rows whose filter ratio dispGeneEst / (0.1 + 1 / baseMean) lies at relative distance 1e-6 below
              and above both bounds of the first round, 1e-4 and 15 — 1e-6 is ten orders above rounding, so the decision is the twin's
              and not an excuse;
  trend-edges-255, -256, -257   one thread short of, exactly and one past a block of trend_pass_kernel: the other 511 blocks are idle
              and must contribute exact zeros (257 rows: S = 4, so the simulated prior runs on this route too);
  trend-edges-tiled   the 599 rows K = 439 times: n = 262 961 > 2 x 512 x 256, every thread of trend_pass_kernel walks its grid-stride
              loop at least twice and some a third time.  In exact arithmetic the coefficients are the base case's (every glm sum scales
              by K), and so are the median and the MAD (an odd repeat of a multiset keeps both middle order statistics): the twin is
              evaluated on the 599 rows.
"""
import numpy as np

import disp_inputs as di
import trend_inputs as ti

from chicdiff_amd import synth

THETAS = [0.0, 0.25, 0.5, 0.75, 1.0]  # the reference's grid
SCANS = {"scan-S4": (1500, 4), "scan-S8": (2051, 8), "scan-S17": (1500, 17)}
SUM_SIZES = (1, 255, 256, 257, 1025)
SUM_OPTS = dict(di.OPTS)
TILE_K = 439
EDGE_SEED = 6300
FILTER_LO, FILTER_HI, FILTER_REL = 1e-4, 15.0, 1e-6
START = (0.1, 1.0)  # the coefficients the first round's filter is formed with
_cache = {}


def _oracle():
    from oracle import oracle as o
    o.build()
    return o


def scan_case(name):
    if name in _cache:
        return _cache[name]
    o = _oracle()
    if name in SCANS:
        n, S = SCANS[name]
        d = synth.make(n, S, fragments=3)
        keep = d["counts"].sum(1) > 0
        _, FM = o.window_sums(None, d["fragFullMean"], d["region_ptr"])
        counts, FM, planted = np.ascontiguousarray(d["counts"][keep], dtype=np.int32), np.ascontiguousarray(FM[keep]), {}
    else:
        base = scan_case("scan-S8")
        counts, FM = base["counts"].copy(), base["FullMean"].copy()
        n, S = counts.shape
        if name == "scan-zero":
            planted = dict(zero=np.array([0, n // 2, n - 1]))
            counts[planted["zero"]] = 0
        elif name == "scan-na":
            partial = (n // 256) * 256  # first row of the partial last tile of prep
            assert 0 < partial < n - 1
            planted = dict(na=[(0, 0), (n - 1, S - 1), (partial, 1)])
            for i, j in planted["na"]:
                FM[i, j] = np.nan
        else:
            raise KeyError(name)
    case = dict(name=name, counts=counts, FullMean=FM, sf=o.size_factors(counts), thetas=list(THETAS), planted=planted)
    _cache[name] = case
    return case


def sum_case(n):
    """The first n rows of scan-S8 with the offsets of theta = 0.5 under the scan's size factors: one design-~1 fit, trend and prior pinned."""
    base = scan_case("scan-S8")
    assert n <= len(base["counts"])
    return dict(name=f"sum-n{n}", counts=np.ascontiguousarray(base["counts"][:n]), FullMean=np.ascontiguousarray(base["FullMean"][:n]), sf=base["sf"],
                theta=0.5, opts=dict(SUM_OPTS), planted={})


def _stage(name, bm, al, S, zero, planted, note):
    c = ti._case(name, bm, al, S, 1, dict(fitType=0), zero=zero, note=note)
    c["planted"] = planted
    return c


def _edges_599():
    n = ti.N
    rng = np.random.default_rng(EDGE_SEED)
    bm, al = ti._trend_columns(rng, n, 0.5, 1e5, sd=0.4)
    zero = np.concatenate([[0], np.arange(260, 330), [n - 1]])
    # below, at and just above 100 minDisp, beside the all-zero rows: (below: no residual; at: a residual, not in the fit; above: in the fit's
    # candidates, and out by the ratio)
    below = np.array([1, 259, 330, n - 2])
    al[below] = [ti.MIN_DISP, np.nextafter(ti.T100, 0.0), ti.MIN_DISP, 0.5 * ti.T100]
    at, above = np.array([2, 331]), np.array([3, 258])
    al[at] = ti.T100
    al[above] = np.nextafter(ti.T100, 1.0)
    # the first round's filter: ratio = dispGeneEst / (0.1 + 1 / baseMean) strictly between 1e-4 and 15
    rows = dict(lo_out=40, lo_in=41, hi_in=300 + 140, hi_out=300 + 141, lo_out2=n - 40, hi_out2=n - 41, lo_in2=500, hi_in2=501)
    for key, i in rows.items():
        bound = FILTER_LO if key.startswith("lo") else FILTER_HI
        inside = "_in" in key
        rel = 1 + FILTER_REL if (bound == FILTER_LO) == inside else 1 - FILTER_REL
        al[i] = bound * rel * (START[0] + START[1] / bm[i])
        assert al[i] > 2 * ti.T100
    planted = dict(zero=zero, below=below, at=at, above=above,
                   out=np.array(sorted(i for k, i in rows.items() if "_out" in k)), inside=np.array(sorted(i for k, i in rows.items() if "_in" in k)))
    return _stage("trend-edges-599", bm, al, 8, zero, planted, "zero runs, 100 minDisp and its neighbours, both filter bounds at 1e-6")


def edge_case(name):
    if name in _cache:
        return _cache[name]
    if name == "trend-edges-599":
        c = _edges_599()
    elif name == "trend-edges-tiled":
        b = edge_case("trend-edges-599")
        n = len(b["baseMean"])
        c = dict(b, name=name, baseMean=np.tile(b["baseMean"], TILE_K), dispGeneEst=np.tile(b["dispGeneEst"], TILE_K), allZero=np.tile(b["allZero"], TILE_K),
                 planted={k: v for k, v in b["planted"].items()}, base="trend-edges-599", copies=TILE_K, note="599 rows x 439: the grid-stride loop wraps twice")
        assert len(c["baseMean"]) == n * TILE_K > 2 * 512 * 256 and TILE_K % 2 == 1
    else:
        n = int(name.rsplit("-", 1)[1])
        assert n in (255, 256, 257)
        rng = np.random.default_rng(EDGE_SEED + n)
        bm, al = ti._trend_columns(rng, n, 0.5, 1e5, sd=0.4)
        below = np.array([1, n - 2])
        al[below] = [ti.MIN_DISP, np.nextafter(ti.T100, 0.0)]
        zero = np.array([0, n - 1])
        c = _stage(name, bm, al, 4 if n == 257 else 8, zero, dict(zero=zero, below=below, at=np.array([], int), above=np.array([], int)),
                   "one block of trend_pass_kernel, 511 idle")
    _cache[name] = c
    return c


EDGES = ["trend-edges-599", "trend-edges-255", "trend-edges-256", "trend-edges-257", "trend-edges-tiled"]
