"""Seeded inputs of the assembly stage (region universe -> N and FullMean per region) at the benchmark's end-to-end shape, for
tests/test_region_assemble.py and tools/assemble_timing.py.

bench.py::end_to_end builds its inputs inside one function, so its recipe is restated here for ONE region set: peaks on the
840 001-fragment map (35 000 fragments per chromosome, every window kept on its bait's chromosome), the device's own region
universe with RUexpand = 5, one sorted (baitID << 32 | otherEndID) -> N table per replicate, random Chicago tables with 2 % NaN
s_i, the distance functions.  Two sources of counts:

  counts="synth"   the benchmark's: chicdiff_amd/synth.py's region counts split over each region's fragments by seeded integer
                   weights (PCG64), pairs with a positive share become a replicate's table.  (The benchmark then gives regions
                   without a read one: its theta scan needs that, the assembly does not, so it is left out.)
  counts="device"  drawn on the device: every replicate keeps a seeded random ``table_share`` of the universe's distinct pairs with
                   counts 1 .. 49 — for shapes whose host-side synthesis would take minutes (20 M peaks x 16 replicates)."""
import numpy as np

MAXFRAG = 840000
CHROM = 35000


def make(ctx, n, S, seed=7, RUexpand=5, counts="synth", table_share=1.0):
    torch = ctx.torch
    dev = ctx.device
    g = torch.Generator(device=dev)
    g.manual_seed(seed)
    nid = MAXFRAG + 1
    chr_of = (torch.arange(0, nid, device=dev) // CHROM).to(torch.int32)
    pb = torch.randint(1000, 800000, (n,), dtype=torch.int64, device=dev, generator=g)
    dd = torch.randint(2, 60, (n,), dtype=torch.int64, device=dev, generator=g) * (torch.randint(0, 2, (n,), device=dev, generator=g) * 2 - 1)
    off_chr = ((pb + dd + RUexpand) // CHROM != pb // CHROM) | ((pb + dd - RUexpand) // CHROM != pb // CHROM)
    po = pb + torch.where(off_chr, -dd, dd)
    key = torch.sort(pb * (1 << 32) + po).values                      # setkey(baitID, oeID)
    pb, po = (key >> 32).to(torch.int32), (key & 0xFFFFFFFF).to(torch.int32)
    del key, dd, off_chr
    ru = ctx.region_universe(pb, po, RUexpand, chr_of)
    bait, oe, ptr = ru["baitID"], ru["otherEndID"], ru["region_ptr"]
    nfrag = int(bait.numel())
    del ru
    rukey = bait.to(torch.int64) * (1 << 32) + oe.to(torch.int64)
    tables = []
    if counts == "synth":
        from chicdiff_amd import synth
        k = torch.from_numpy(np.ascontiguousarray(synth.make(n, S)["counts"].T)).to(dev)
        wrng = np.random.Generator(np.random.PCG64(20190123 + seed))
        cnt = ptr[1:] - ptr[:-1]
        rid = torch.repeat_interleave(torch.arange(n, device=dev), cnt)
        w = torch.from_numpy(np.minimum(wrng.standard_gamma(0.3, nfrag) * 4096.0, 2.0 ** 30).astype(np.int64) + 1).to(dev)
        cum = torch.cumsum(w, 0)
        cum_excl = cum - w
        start = cum_excl[ptr[:-1].clamp(max=nfrag - 1)]
        tot = (cum[(ptr[1:] - 1).clamp(min=0)] - start).to(torch.float64)
        hi = (cum - start[rid]).to(torch.float64) / tot[rid]
        lo = (cum_excl - start[rid]).to(torch.float64) / tot[rid]
        del w, cum, cum_excl, start, tot
        for j in range(S):
            kj = k[j][rid].to(torch.float64)
            v = (torch.floor(kj * hi + 1e-9) - torch.floor(kj * lo + 1e-9)).to(torch.int32)
            sel = v > 0
            ks, order = torch.sort(rukey[sel])
            vs = v[sel][order]
            first = torch.ones_like(ks, dtype=torch.bool)
            first[1:] = ks[1:] != ks[:-1]                             # a pair that sits in several regions keeps one count
            tables.append((ks[first].contiguous(), vs[first].contiguous()))
        del hi, lo, rid, k
    elif counts == "device":
        uniq = torch.unique(rukey)                                    # sorted
        for j in range(S):
            keep = torch.rand(uniq.numel(), device=dev, generator=g) < table_share
            ks = uniq[keep].contiguous()
            tables.append((ks, torch.randint(1, 50, (ks.numel(),), dtype=torch.int32, device=dev, generator=g)))
        del uniq
    else:
        raise ValueError(counts)
    del rukey
    sj = torch.exp(torch.randn((S, nid), dtype=torch.float64, device=dev, generator=g) * 0.3)
    si = torch.exp(torch.randn((S, nid), dtype=torch.float64, device=dev, generator=g) * 0.3)
    si[torch.rand((S, nid), device=dev, generator=g) < 0.02] = float("nan")   # other ends Chicago never saw: s_i NA -> 1
    ntblb, ntlb = 6, 6
    tblb = torch.randint(0, ntblb, (S, nid), dtype=torch.int32, device=dev, generator=g)
    tlb = torch.randint(0, ntlb, (S, nid), dtype=torch.int32, device=dev, generator=g)
    T = torch.exp(torch.randn((S, ntblb, ntlb), dtype=torch.float64, device=dev, generator=g) * 0.5 - 3.0)
    midsum = torch.arange(nid, device=dev, dtype=torch.int64) * 8000 + 4000
    distfun = np.zeros((S, 10))
    for j in range(S):
        fit = np.array([14.0 + 0.1 * j, -1.6, 0.05, -0.003])
        ends = np.array([np.log(10000.0), np.log(1.5e6)])
        beta = fit[1] + 2 * fit[2] * ends + 3 * fit[3] * ends ** 2
        alpha = fit[0] + (fit[1] - beta) * ends + fit[2] * ends ** 2 + fit[3] * ends ** 3
        distfun[j] = [*fit, alpha[0], beta[0], alpha[1], beta[1], ends[0], ends[1]]
    return dict(bait=bait, oe=oe, region_ptr=ptr, tables=tables, id_min=0, midsum=midsum, sj=sj, si=si, tblb=tblb, tlb=tlb, T=T,
                distfun=distfun, n=n, S=S, nfrag=nfrag)


def background_args(d):
    """The arguments region_assemble and fragment_background share, in their order."""
    return (d["id_min"], d["midsum"], d["sj"], d["si"], d["tblb"], d["tlb"], d["T"], d["distfun"])


def three_calls(ctx, bait, oe, region_ptr, tables, bg):
    """The path region_assemble replaces: count_join_multi -> fragment_background(only_fullmean=True) -> window_sums."""
    fragN = ctx.count_join_multi(bait, oe, tables)
    _, _, fragFM = ctx.fragment_background(bait, oe, *bg, only_fullmean=True)
    return ctx.window_sums(fragN, fragFM, region_ptr)


def assemble(ctx, bait, oe, region_ptr, tables, bg, **kw):
    return ctx.region_assemble(bait, oe, region_ptr, tables, *bg, **kw)
