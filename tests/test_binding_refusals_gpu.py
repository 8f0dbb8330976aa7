"""Every public method of HipContext that takes a caller's tensor refuses a malformed one with ValueError, naming the argument,
BEFORE any entry point of the C ABI is reached (chicdiff_amd/hip.py, the marshalling layer).  One table: per method a well-formed
call at the smallest meaningful shape (n = 64 rows, S = 4 with group [0, 0, 1, 1], 100 RU rows in 2 regions, tables of 50 keys, a
16-fragment map) and, one argument at a time, its corruptions: the neighbouring dtype at the same shape, the tensor on the CPU, a
strided view of the right shape, one element short, S off by one; for table lists unequal lengths, 0 and 65 tables; for ``want`` an
unknown name and a buffer of the wrong dtype; for ``group`` length S - 1.  The context's library is replaced by a proxy that raises
as soon as any entry point is looked up, so nothing is launched; the well-formed call must reach it (the guard on the guard)."""
import inspect

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
S, N, NRU, NID, NK = 4, 64, 100, 16, 50
GROUP = [0, 0, 1, 1]


class Reached(AssertionError):
    pass


class NoLaunch:
    """The context's library with every entry point but the error text (and the destructor) walled off."""

    def __init__(self, lib):
        self._lib = lib

    def __getattr__(self, name):
        if name in ("chicdiff_hip_last_error", "chicdiff_hip_destroy"):
            return getattr(self._lib, name)
        raise Reached(f"the entry point was reached: {name}")


@pytest.fixture(scope="module")
def ctx():
    import __graft_entry__ as g
    g.build()
    from chicdiff_amd import hip
    c = hip.HipContext(0)
    yield c
    c.close()


class Inputs:
    def __init__(self, ctx):
        import torch
        from chicdiff_amd import hip
        dev = ctx.device
        rng = np.random.default_rng(7)
        t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
        i32 = lambda hi, *shape: t(rng.integers(0, hi, shape).astype(np.int32))
        f64 = lambda *shape: t(rng.uniform(0.1, 1.0, shape))
        self.counts, self.nf = i32(50, S, N), f64(S, N)
        self.bait, self.oe, self.ptr = i32(NID, NRU), i32(NID, NRU), t(np.array([0, 40, NRU], dtype=np.int64))
        self.keys, self.vals = t(np.sort(rng.choice(1 << 20, NK, replace=False)).astype(np.int64)), i32(9, NK)
        self.tables = [(self.keys, self.vals)] * S
        self.midsum, self.chr = t(np.arange(NID, dtype=np.int64) * 8000 + 4000), t(np.zeros(NID, dtype=np.int32))
        self.sj, self.si, self.tblb, self.tlb, self.T = f64(S, NID), f64(S, NID), i32(3, S, NID), i32(3, S, NID), f64(S, 3, 3)
        self.distfun = np.ones((S, 10))
        self.fragN, self.fragFM = i32(5, S, NRU), f64(S, NRU)
        self.p, self.cov, self.argmax = f64(N), f64(N), i32(S, N)
        self.flags = t(np.ones(NID + 1, dtype=np.uint8))
        self.text = t(np.frombuffer(b"1\t2\t3\n" * 8, dtype=np.uint8).copy())
        self.rep = (i32(NID, N), i32(NID, N), i32(9, N), f64(N), f64(N), f64(N))
        self.cols = [i32(9, N), f64(N)]
        info = dict(zip(hip.PEAKS_INFO, [0] * len(hip.PEAKS_INFO)), nrows=N, nscore=2, maxbait=NID)
        self.peaks = [hip.Peaks(dict(info), i32(NID, 6, N), f64(N), f64(2, N), t(np.arange(N, dtype=np.int64)), score_names=["a", "b"]) for _ in range(2)]
        for pk in self.peaks:
            pk.chr_keys, pk.name_hash = t(np.zeros((2, N), dtype=np.int64)), t(np.zeros((2, N), dtype=np.int64))
        self.torch = torch

    def out(self, dtype, *shape):
        return self.torch.empty(shape, dtype=dtype, device=self.counts.device)


def table_cases(v):
    k, w = v.keys, v.vals
    rest = v.tables[1:]
    return [("tables: dtype of vals", "tables[0] vals:", dict(tables=[(k, w.long())] + rest)),
            ("tables: dtype of keys", "tables[0] keys:", dict(tables=[(k.int(), w)] + rest)),
            ("tables: keys on the CPU", "tables[0] keys:", dict(tables=[(k.cpu(), w)] + rest)),
            ("tables: strided vals", "tables[0] vals:", dict(tables=[(k, strided(w))] + rest)),
            ("tables: len(keys) != len(vals)", "tables[0]:", dict(tables=[(k, w[:-1])] + rest)),
            ("tables: 0", "S <= 64", dict(tables=[])),
            ("tables: 65", "S <= 64", dict(tables=[(k, w)] * 65))]


def fit_cases(v, other):
    f32 = v.torch.float32
    return [("group: S - 1", "group:", dict(group=GROUP[:-1])),
            ("S off by one", other, dict(d_counts=v.out(v.torch.int32, S + 1, N))),
            ("want: unknown name", "want:", dict(want=["pvalue", "pvalues"])),
            ("outputs: dtype of a buffer", "outputs['pvalue']:", dict(want=["pvalue"], outputs=dict(pvalue=v.out(f32, N)))),
            ("outputs: a buffer one short", "outputs['pvalue']:", dict(want=["pvalue"], outputs=dict(pvalue=v.out(v.torch.float64, N - 1))))]


def column_cases(v):
    a, b = v.cols
    return [("columns: dtype", "columns[1]:", dict(columns=[a, b.float()])), ("columns: on the CPU", "columns[0]:", dict(columns=[a.cpu(), b])),
            ("columns: strided", "columns[1]:", dict(columns=[a, strided(b)])), ("columns: one short", "columns[1]:", dict(columns=[a, b[:-1]]))]


def rep_cases(v):
    r = v.rep
    sub = lambda k, t: dict(reps=[r[:k] + (t,) + r[k + 1:], r])
    return [("reps: dtype", "reps[0].N:", sub(2, r[2].long())), ("reps: on the CPU", "reps[0].Bmean:", sub(3, r[3].cpu())),
            ("reps: strided", "reps[0].score:", sub(4, strided(r[4]))), ("reps: one short", "reps[0].distSign:", sub(5, r[5][:-1])),
            ("reps: none", "countput:", dict(reps=[]))]


def peaks_with(v, f, **columns):
    import copy
    pks = [copy.copy(pk) for pk in v.peaks]
    for name, t in columns.items():
        setattr(pks[f], name, t)
    return pks


def peaks_cases(v, columns, who, arg):
    """Every column of a Peaks the method reads, of file 0: the neighbouring dtype, on the CPU, one row short.  (No strided case: the
    columns of a merged Peaks ARE views, and the two methods lay them out themselves before the rule sees them.)"""
    torch = v.torch
    neighbour = {torch.float64: torch.float32, torch.int32: torch.int64, torch.int64: torch.int32}
    cases = []
    for name in columns:
        t = getattr(v.peaks[0], name)
        for tag, bad in (("dtype", t.to(neighbour[t.dtype])), ("on the CPU", t.cpu()), ("one short", t[..., :-1])):
            cases.append((f"{name}: {tag}", who.format(name), dict(peaks=arg(peaks_with(v, 0, **{name: bad})))))
    return cases


# method -> (well-formed keyword arguments; {argument: whose name the refusal carries when that argument is one element short — itself
# unless listed, None where a shorter tensor is a well-formed smaller problem}; further corruptions as (tag, text expected, arguments))
ROWS = {
    "size_factors": lambda v: (dict(d_counts=v.counts), dict(d_counts=None), []),
    "offsets": lambda v: (dict(d_fullmean=v.nf, size_factors=np.ones(S), out=v.out(v.torch.float64, S, N)), dict(d_fullmean="out:"),
                          [("size_factors: S - 1", "size_factors:", dict(size_factors=np.ones(S - 1))),
                           ("S off by one", "size_factors:", dict(d_fullmean=v.out(v.torch.float64, S + 1, N)))]),
    "window_sums": lambda v: (dict(d_fragN=v.fragN, d_fragFM=v.fragFM, d_region_ptr=v.ptr), dict(d_fragN="d_fragFM:", d_region_ptr=None),
                              [("S off by one", "d_fragFM:", dict(d_fragN=v.out(v.torch.int32, S + 1, NRU)))]),
    "count_join": lambda v: (dict(d_bait=v.bait, d_oe=v.oe, d_keys=v.keys, d_vals=v.vals), dict(d_bait="d_oe:", d_keys="d_vals:"), []),
    "count_join_multi": lambda v: (dict(d_bait=v.bait, d_oe=v.oe, tables=v.tables, out=v.out(v.torch.int32, S, NRU)), dict(d_bait="d_oe:"),
                                   table_cases(v) + [("S off by one", "out:", dict(tables=v.tables + v.tables[:1]))]),
    "count_join_inner": lambda v: (dict(d_bait=v.bait, d_oe=v.oe, tables=v.tables), dict(d_bait="d_oe:"), table_cases(v)),
    "region_assemble": lambda v: (
        dict(d_bait=v.bait, d_oe=v.oe, d_region_ptr=v.ptr, tables=v.tables, id_min=0, d_midsum=v.midsum, d_sj=v.sj, d_si=v.si, d_tblb=v.tblb,
             d_tlb=v.tlb, d_T=v.T, distfun=v.distfun),
        dict(d_bait="d_oe:", d_region_ptr=None, d_midsum="d_sj:", d_T=None),
        table_cases(v) + [("distfun: shape", "distfun:", dict(distfun=v.distfun[:, :9])), ("S off by one", "d_sj:", dict(tables=v.tables[:-1]))]),
    "region_avdist": lambda v: (dict(d_bait=v.bait, d_oe=v.oe, d_region_ptr=v.ptr, id_min=0, d_midsum=v.midsum, d_chr=v.chr),
                                dict(d_bait="d_oe:", d_region_ptr=None, d_midsum="d_chr:"), []),
    "fragment_background": lambda v: (
        dict(d_bait=v.bait, d_oe=v.oe, id_min=0, d_midsum=v.midsum, d_sj=v.sj, d_si=v.si, d_tblb=v.tblb, d_tlb=v.tlb, d_T=v.T, distfun=v.distfun),
        dict(d_bait="d_oe:", d_midsum="d_sj:", d_T=None),
        [("distfun: S - 1", "distfun:", dict(distfun=v.distfun[:-1])), ("S off by one", "d_si:", dict(d_sj=v.out(v.torch.float64, S + 1, NID)))]),
    "count_table": lambda v: (dict(d_bait=v.bait, d_oe=v.oe, d_N=v.fragN[0].contiguous(), d_bait_in_RU=v.flags),
                              dict(d_bait="d_oe:", d_bait_in_RU=None), []),
    "read_chinput": lambda v: (dict(path="no such file.chinput", d_bait_in_RU=v.flags), dict(d_bait_in_RU=None), []),
    "parse_chinput_text": lambda v: (dict(d_text=v.text, cols=(0, 1, 2)), dict(d_text=None), []),
    "parse_peaks_text": lambda v: (dict(d_text=v.text, sep="\t", score_cols=[11]), dict(d_text=None), []),
    "filter_peaks": lambda v: (dict(peaks=v.peaks[0], score=5.0, cond_of_col=[0, 1], replicate_rule=False), {},
                               peaks_cases(v, ("baitID", "oeID", "dist", "scores"), "peaks.{}:", lambda pks: pks[0])),
    "merge_peaks": lambda v: (dict(peaks=v.peaks), {},
                              peaks_cases(v, ("ints", "dist", "scores", "chr_keys", "name_hash"), "peaks[0].{}:", lambda pks: pks)),
    "cooks_filter": lambda v: (dict(d_counts=v.counts, group=GROUP, d_maxCooks=v.p, d_cooksArgmax=v.argmax, d_pvalue=v.cov, cutoff=1.0),
                               dict(d_counts="d_maxCooks:"),
                               [("group: S - 1", "group:", dict(group=GROUP[:-1])), ("S off by one", "group:", dict(d_counts=v.out(v.torch.int32, S + 1, N)))]),
    "independent_filtering": lambda v: (dict(d_baseMean=v.cov, d_pvalue=v.p), dict(d_pvalue="d_baseMean:"), []),
    "bh_adjust": lambda v: (dict(d_p=v.p), dict(d_p=None), []),
    "ihw_apply": lambda v: (dict(d_avDist=v.cov, d_pvalue=v.p, breaks=[0.0, 1.0, 2.0, 3.0, np.inf], avWeights=[1.5, 1.0, 1.0, 0.5]),
                            dict(d_avDist="d_pvalue:"), [("breaks: one short", "breaks:", dict(breaks=[0.0, 1.0, 2.0, np.inf]))]),
    "ihw_train": lambda v: (dict(d_pvalue=v.p, d_covariate=v.cov), dict(d_pvalue="d_covariate:"), [("seed: negative", "seed", dict(seed=-1))]),
    "selftest_ihw_knots": lambda v: (dict(d_pvalue=v.p, d_covariate=v.cov), dict(d_pvalue="d_covariate:"), [("seed: a bool", "seed", dict(seed=True))]),
    "region_universe": lambda v: (dict(d_bait=v.bait, d_oe=v.oe, RUexpand=1, d_chr_of=v.chr), dict(d_bait="d_oe:", d_chr_of=None), []),
    "candidate_interactions": lambda v: (
        dict(d_baitID=v.bait[:N].contiguous(), d_minOE=v.oe[:N].contiguous(), d_maxOE=v.oe[:N].contiguous(), d_p=v.p, d_peak_baitID=v.bait[:10].contiguous(),
             d_peak_oeID=v.oe[:10].contiguous(), d_scores=v.fragFM[:2, :10].contiguous(), ncond1=1, ncond2=1, merged=False, score=5.0, pvcut=0.05,
             minDeltaAsinhScore=1.0),
        dict(d_baitID="d_minOE:", d_scores="d_peak_baitID:"),
        [("pair_row: dtype", "pair_row:", dict(pair_row=v.out(v.torch.int64, 100))), ("pair_row: on the CPU", "pair_row:", dict(pair_row=v.out(v.torch.int32, 100).cpu()))]),
    "control_draws": lambda v: (
        dict(d_ru_baitID=v.bait, d_region_ptr=v.ptr, d_minOE=v.oe[:2].contiguous(), d_maxOE=v.oe[2:4].contiguous(), d_bmap_id=v.bait[:8].contiguous(),
             d_bmap_chr=v.chr[:8].contiguous(), chr_min=[0], chr_max=[NID - 1], seed=1),
        dict(d_ru_baitID=None, d_region_ptr="d_minOE:", d_bmap_id="d_bmap_chr:"), [("seed: 2^64", "seed", dict(seed=1 << 64))]),
    "chicago_tables": lambda v: (
        dict(d_bait=v.rep[0], d_oe=v.rep[1], d_s_j=v.p, d_s_i=v.cov, d_Tmean=v.rep[3], d_refBinMean=v.rep[4], d_tblb=v.rep[2], d_tlb=v.rep[2],
             d_distbin=v.rep[2], id_min=0, ndistbin=9, sj=v.out(v.torch.float64, NID), si=v.out(v.torch.float64, NID),
             tblb_of=v.out(v.torch.int32, NID), tlb_of=v.out(v.torch.int32, NID), T=v.out(v.torch.float64, 3, 3)),
        dict(d_bait="d_oe:", sj="si:", T=None), []),
    "countput": lambda v: (dict(reps=[v.rep, v.rep], id_min=0, d_midsum=v.midsum, d_chr=v.chr), dict(d_midsum="d_chr:"), rep_cases(v)),
    "table_text": lambda v: (dict(columns=v.cols), {}, column_cases(v)),
    "write_table": lambda v: (dict(path="never written.csv", columns=v.cols, header=["a", "b"]), {}, column_cases(v)),
    "selftest_format_double_dev": lambda v: (dict(d_x=v.p), dict(d_x=None), []),
    "nbglm_fit": lambda v: (dict(d_counts=v.counts, d_nf=v.nf, group=GROUP), dict(d_counts="d_nf:"), fit_cases(v, "d_nf:")),
    "wald_test": lambda v: (dict(d_counts=v.counts, d_fullmean=v.nf, group=GROUP), dict(d_counts="d_fullmean:"), fit_cases(v, "d_fullmean:")),
    "nbglm_fit_host": lambda v: (dict(counts=np.ones((N, S), dtype=np.int32), nf=np.ones((N, S)), group=GROUP), {},
                                 [("group: S - 1", "group:", dict(group=GROUP[:-1])), ("want: unknown name", "want:", dict(want=["padj"])),
                                  ("nf: one row short", "nf", dict(nf=np.ones((N - 1, S))))]),
    "theta_grid": lambda v: (dict(d_counts=v.counts, d_fullmean=v.nf, size_factors=np.ones(S), thetas=[0.0, 0.5]), dict(d_counts="d_fullmean:"),
                             [("size_factors: S - 1", "size_factors:", dict(size_factors=np.ones(S - 1))),
                              ("S off by one", "d_fullmean:", dict(d_counts=v.out(v.torch.int32, S + 1, N)))]),
    "selftest_math": lambda v: (dict(op=0, d_x=v.p), dict(d_x=None), []),
    "selftest_landau": lambda v: (dict(d_z=v.p), dict(d_z=None), []),
    "selftest_math3": lambda v: (dict(op=12, d_x=v.p, d_y=v.cov), dict(d_x="d_y:"), []),
    "selftest_objective": lambda v: (dict(d_counts=v.counts, d_nf=v.nf, group=GROUP, d_log_alpha=v.fragFM[:3, :N].t().contiguous(), d_prior_mean=v.p),
                                     dict(d_counts="d_nf:", d_log_alpha=None),
                                     [("group: S - 1", "group:", dict(group=GROUP[:-1])),
                                      ("S off by one", "d_nf:", dict(d_counts=v.out(v.torch.int32, S + 1, N)))]),
    "selftest_global_stage": lambda v: (dict(d_baseMean=v.p, d_dispGeneEst=v.cov, d_allZero=v.argmax, S=S, p=2),
                                        dict(d_baseMean="d_dispGeneEst:"), []),
    "selftest_resid_hist": lambda v: (dict(d_resid=v.p), dict(d_resid=None), []),
    "wald_pvalues": lambda v: (dict(d_stat=v.p), dict(d_stat=None), []),
}


def strided(t):
    """a view of t's shape and values' dtype that is not contiguous"""
    wide = t.new_zeros(t.shape[:-1] + (2 * t.shape[-1],))
    view = wide[..., ::2]
    assert view.shape == t.shape and not view.is_contiguous()
    return view


def corruptions(v, kwargs, short):
    torch = v.torch
    neighbour = {torch.float64: torch.float32, torch.int32: torch.int64, torch.int64: torch.int32, torch.uint8: torch.int8}
    for name, t in kwargs.items():
        if not torch.is_tensor(t):
            continue
        yield f"{name}: dtype", name + ":", {name: t.to(neighbour[t.dtype])}
        yield f"{name}: on the CPU", name + ":", {name: t.cpu()}
        yield f"{name}: strided", name + ":", {name: strided(t)}
        who = short.get(name, name + ":")
        if who is not None:
            yield f"{name}: one short", who, {name: t[..., :-1].contiguous()}


@pytest.fixture(scope="module")
def inputs(ctx):
    return Inputs(ctx)


@pytest.mark.parametrize("method", sorted(ROWS))
def test_refusal_comes_before_any_entry_point(ctx, inputs, method):
    kwargs, short, extra = ROWS[method](inputs)
    call = getattr(ctx, method)
    lib = ctx.lib
    ctx.lib = NoLaunch(lib)
    try:
        with pytest.raises(Reached):                                   # the guard itself: the well-formed call does reach the library
            call(**kwargs)
        cases = list(corruptions(inputs, kwargs, short)) + extra
        assert cases, method
        for tag, who, change in cases:
            with pytest.raises(ValueError) as e:                       # (Reached is an AssertionError: an entry point reached fails here)
                call(**{**kwargs, **change})
            assert who in str(e.value), (method, tag, str(e.value))
    finally:
        ctx.lib = lib


def test_every_method_that_takes_tensors_has_a_row():
    from chicdiff_amd import hip
    listed = ("tables", "reps", "columns", "outputs")
    missing = []
    for name, fn in inspect.getmembers(hip.HipContext, inspect.isfunction):
        params = inspect.signature(fn).parameters
        if not name.startswith("_") and any(p.startswith("d_") or p in listed for p in params) and name not in ROWS:
            missing.append(name)
    assert not missing, missing
    assert all(hasattr(hip.HipContext, name) for name in ROWS)
