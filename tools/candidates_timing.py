"""getCandidateInteractions' device path (chicdiff_hip_candidate_interactions_dev) at the benchmark's scale, beside the host time of
the same computation written as vectorised numpy.

    python3 tools/candidates_timing.py [--shapes 2000000x8,250000x8] [--reps 7] [--out FILE] [--no-host]
    python3 tools/candidates_timing.py --merge-stats KERNEL_STATS.csv --out FILE      # append rocprofv3's per-kernel figures
    python3 tools/candidates_timing.py --method hmp ...                               # time method = "hmp" (default "min")
    python3 tools/candidates_timing.py --ab [--parent-lib OLD.so] --out FILE          # A/B lines instead, see below

--ab: in one process, alternating within each repeat, device events around the raw C-ABI calls on buffers allocated once:
(a) method "min" through chicdiff_hip_candidate_interactions_dev of this build against the same entry point of --parent-lib (an
earlier build of the library, loaded beside this one with a context of its own on the same stream), and (b) "hmp" against "min"
through chicdiff_hip_candidate_interactions_method_dev of this build.  One JSON line per shape with the repeats, medians and ranges.

Geometry: the synthetic generator's of tests/assemble_inputs.py — peaks on an 840 001-fragment map, the device's own region
universe with RUexpand = 5 as the region table (one region per peak, span <= 10), handed over in random row order; S log-normal
score columns and uniform^4 p values, 2 % NaN in both.  Two device figures per repeat: ``events`` = device events around the
binding's call (allocations of the outputs and the read-back of the two counts included), ``kernels`` = the library's own timer
around everything it enqueues.  ``host_numpy_ms`` is what it says: one run of the numpy form on this host's CPU, no R involved.
One JSON line per shape.  Under rocprofv3 (--kernel-trace --stats, a run of its own) use --reps 1 --no-host; the overlap
kernel's algorithmic bytes are in the line (``overlap_bytes``) to set beside its time."""
import argparse
import csv
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

ap = argparse.ArgumentParser()
ap.add_argument("--shapes", default="2000000x8,250000x8")
ap.add_argument("--reps", type=int, default=7)
ap.add_argument("--out", default=None)
ap.add_argument("--no-host", action="store_true")
ap.add_argument("--merge-stats", default=None)
ap.add_argument("--method", default="min", choices=["min", "hmp"])
ap.add_argument("--ab", action="store_true")
ap.add_argument("--parent-lib", default=None)
args = ap.parse_args()


def emit(line):
    print(json.dumps(line))
    if args.out:
        with open(args.out, "a") as f:
            f.write(json.dumps(line) + "\n")


if args.merge_stats:
    # the entry point's own kernels: cand_*, and rocPRIM's under the library's version namespace (the set-up of this tool sorts through
    # torch, whose rocPRIM carries another one) — the namespace of the 32-bit-key pair sort, which only the library launches
    import re
    rows = list(csv.DictReader(open(args.merge_stats)))
    tag = lambda name: (re.findall(r"ROCPRIM_\d+_NS", name) or [""])[0]
    ours = {tag(r["Name"]) for r in rows if "rocprim" in r["Name"] and "unsigned int, int" in r["Name"]}
    rows = [r for r in rows if "cand_" in r["Name"] or ("rocprim" in r["Name"] and tag(r["Name"]) in ours)]
    short = lambda name: re.sub(r"^.*(cand_\w+).*$", r"\1", name) if "cand_" in name else "rocprim " + " ".join(
        re.findall(r"(onesweep_iteration|onesweep_global_offsets|lookback_scan\w*|init_lookback_scan_state)\w*", name)[-1:] +
        re.findall(r"default_config, ([\w ]+(?:, \w+)?)>", name)[:1])
    emit(dict(kernel_stats=[dict(name=short(r["Name"]), calls=int(r["Calls"]), total_us=float(r["TotalDurationNs"]) / 1e3,
                                 avg_us=float(r["AverageNs"]) / 1e3) for r in rows],
              total_us=sum(float(r["TotalDurationNs"]) for r in rows) / 1e3, source="rocprofv3 --kernel-trace --stats, 2000000x8, one call",
              note="one of the int64 scans (and of the scan-state initialisations) belongs to the set-up's region_universe call"))
    sys.exit(0)

import torch  # noqa: E402

from chicdiff_amd import hip  # noqa: E402

SCORE, PVCUT, MIND = 5.0, 0.05, 1.0
MAXFRAG, CHROM = 840000, 35000


def make(ctx, n, S, seed=7):
    dev = ctx.device
    g = torch.Generator(device=dev)
    g.manual_seed(seed)
    chr_of = (torch.arange(0, MAXFRAG + 1, device=dev) // CHROM).to(torch.int32)
    pb = torch.randint(1000, 800000, (n,), dtype=torch.int64, device=dev, generator=g)
    dd = torch.randint(2, 60, (n,), dtype=torch.int64, device=dev, generator=g) * (torch.randint(0, 2, (n,), device=dev, generator=g) * 2 - 1)
    off = ((pb + dd + 5) // CHROM != pb // CHROM) | ((pb + dd - 5) // CHROM != pb // CHROM)
    key = torch.unique(pb * (1 << 32) + pb + torch.where(off, -dd, dd))       # one peak matrix row per pair
    key = key[torch.randperm(key.numel(), device=dev, generator=g)]
    pb, po = (key >> 32).to(torch.int32), (key & 0xFFFFFFFF).to(torch.int32)
    ru = ctx.region_universe(pb, po, 5, chr_of)
    perm = torch.randperm(pb.numel(), device=dev, generator=g)               # the results table is not in key order
    rb, lo, hi = pb[perm].contiguous(), ru["minOE"][perm].contiguous(), ru["maxOE"][perm].contiguous()
    ok = lo > -(1 << 31)
    rb, lo, hi = rb[ok].contiguous(), lo[ok].contiguous(), hi[ok].contiguous()
    p = torch.rand(rb.numel(), dtype=torch.float64, device=dev, generator=g) ** 4
    p[torch.rand(rb.numel(), device=dev, generator=g) < 0.02] = float("nan")
    s = torch.exp(1.5 + torch.randn((S, pb.numel()), dtype=torch.float64, device=dev, generator=g))
    s[torch.rand(s.shape, device=dev, generator=g) < 0.02] = float("nan")
    return dict(baitID=rb, minOE=lo, maxOE=hi, p=p, peak_baitID=pb, peak_oeID=po, scores=s)


def numpy_form(bait, minOE, maxOE, p, pb, po, scores, nc1, score, pvcut, mind):
    """The twin's statements as whole-array numpy: lexsort of the regions, two searchsorted per selected peak over the look-back
    window, expansion of the candidate ranges, min by group.  (ngroups, npairs)."""
    with np.errstate(invalid="ignore"):
        sel = (scores > score).any(axis=0)
    delta = np.abs(np.arcsinh(scores[:nc1].mean(axis=0)) - np.arcsinh(scores[nc1:].mean(axis=0)))
    order = np.lexsort((maxOE, minOE, bait))
    sb, slo, shi = bait[order].astype(np.int64), minOE[order].astype(np.int64), maxOE[order]
    rk = (sb << 32) + slo
    span = int((shi - slo).max())
    idx = np.flatnonzero(sel)
    pk = (pb[idx].astype(np.int64) << 32) + po[idx]
    o = np.argsort(pk, kind="stable")
    idx, pk = idx[o], pk[o]
    a, b = np.searchsorted(rk, pk - span, "left"), np.searchsorted(rk, pk, "right")
    cnt = b - a
    owner = np.repeat(np.arange(len(idx)), cnt)
    j = np.arange(int(cnt.sum())) - np.repeat(np.cumsum(cnt) - cnt, cnt) + np.repeat(a, cnt)
    ok = (shi[j] >= po[idx][owner]) & (sb[j] == pb[idx][owner])
    owner, rows = owner[ok], order[j[ok]]
    deg = np.bincount(owner, minlength=len(idx))
    has = deg > 0
    starts = (np.cumsum(deg) - deg)[has]
    minp = np.minimum.reduceat(p[rows], starts) if len(rows) else np.zeros(0)     # np.minimum carries NaN, as min() without na.rm
    with np.errstate(invalid="ignore"):
        keep = (minp <= pvcut) & (delta[idx][has] >= mind)
    return int(keep.sum()), int(deg[has][keep].sum())


def ab(ctx, d, S, shape):
    """The A/B lines of --ab for one shape."""
    import ctypes as C
    nc1, P, nreg = S // 2, d["peak_baitID"].numel(), d["baitID"].numel()
    dev = ctx.device
    gpeak, gptr = torch.empty(P, dtype=torch.int32, device=dev), torch.empty(P + 1, dtype=torch.int64, device=dev)
    gmin, gdelta = (torch.empty(P, dtype=torch.float64, device=dev) for _ in range(2))
    pairs = torch.empty(16 * P, dtype=torch.int32, device=dev)
    ng, npairs = C.c_int64(0), C.c_int64(0)
    head = [d[k].data_ptr() for k in ("baitID", "minOE", "maxOE", "p")] + [nreg] + [d[k].data_ptr() for k in ("peak_baitID", "peak_oeID", "scores")] + [
        P, S, nc1, S - nc1, 0, SCORE, PVCUT, MIND]
    tail = [pairs.numel(), gpeak.data_ptr(), gptr.data_ptr(), gmin.data_ptr(), gdelta.data_ptr(), pairs.data_ptr(), C.byref(ng), C.byref(npairs)]
    runs = {"min_old_entry": lambda: ctx.lib.chicdiff_hip_candidate_interactions_dev(ctx.h, *head, *tail),
            "min": lambda: ctx.lib.chicdiff_hip_candidate_interactions_method_dev(ctx.h, *head, 0, *tail),
            "hmp": lambda: ctx.lib.chicdiff_hip_candidate_interactions_method_dev(ctx.h, *head, 1, *tail)}
    if args.parent_lib:
        old = C.CDLL(os.path.abspath(args.parent_lib))
        old.chicdiff_hip_create.argtypes = [C.POINTER(C.c_void_p), C.c_int32]
        old.chicdiff_hip_set_stream.argtypes = [C.c_void_p, C.c_void_p]
        old.chicdiff_hip_destroy.argtypes = [C.c_void_p]
        old.chicdiff_hip_candidate_interactions_dev.argtypes = ctx.lib.chicdiff_hip_candidate_interactions_dev.argtypes
        oh = C.c_void_p()
        assert old.chicdiff_hip_create(C.byref(oh), 0) == 0
        assert old.chicdiff_hip_set_stream(oh, C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)) == 0
        runs["min_parent_lib"] = lambda: old.chicdiff_hip_candidate_interactions_dev(oh, *head, *tail)
    ms, counts = {k: [] for k in runs}, {}
    for rep_ in range(args.reps + 2):   # two warm-up rounds
        for k, f in runs.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            rc = f()
            e1.record()
            torch.cuda.synchronize()
            assert rc == 0, (k, rc)
            counts[k] = [ng.value, npairs.value]
            if rep_ >= 2:
                ms[k].append(e0.elapsed_time(e1))
    emit(dict(ab=True, shape=shape, regions=nreg, peaks=P, reps=args.reps, order=list(runs), counts=counts, events_ms=ms,
              median_ms={k: float(np.median(v)) for k, v in ms.items()}, range_ms={k: [min(v), max(v)] for k, v in ms.items()}))
    if args.parent_lib:
        old.chicdiff_hip_destroy(oh)


ctx = hip.HipContext(0)
ctx.enable_timing(not args.ab)
for shape in args.shapes.split(","):
    n, S = (int(x) for x in shape.split("x"))
    d = make(ctx, n, S)
    if args.ab:
        ab(ctx, d, S, shape)
        del d
        continue
    nc1 = S // 2
    call = lambda: ctx.candidate_interactions(d["baitID"], d["minOE"], d["maxOE"], d["p"], d["peak_baitID"], d["peak_oeID"], d["scores"],
                                              nc1, S - nc1, False, SCORE, PVCUT, MIND, method=args.method)
    for _ in range(2 if args.reps > 1 else 0):
        call()
    events, kernels = [], []
    for _ in range(args.reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        r = call()
        e1.record()
        torch.cuda.synchronize()
        events.append(e0.elapsed_time(e1))
        kernels.append(ctx.last_candidates_ms)
    nreg, P = d["baitID"].numel(), d["peak_baitID"].numel()
    nsel = int((d["scores"] > SCORE).any(dim=0).sum())
    line = dict(shape=shape, method=args.method, regions=nreg, peaks=P, selected=nsel, ngroups=r["ngroups"], npairs=r["npairs"], reps=args.reps,
                events_ms=events, kernels_ms=kernels, events_median_ms=float(np.median(events)), kernels_median_ms=float(np.median(kernels)),
                kernels_min_ms=min(kernels), kernels_max_ms=max(kernels),
                # cand_overlap_kernel: per region key 8 + row 4 + maxOE 4 + p 8 read; per selected peak key 8 + row 4 + delta 8 read and
                # keep 4 + kept degree 8 + min p 8 + first 4 + mask 8 written; per dropped peak 8 read, 12 written
                overlap_bytes=dict(read=24 * nreg + 20 * nsel + 8 * (P - nsel), written=32 * nsel + 12 * (P - nsel)))
    if not args.no_host:
        h = {k: v.cpu().numpy() for k, v in d.items()}
        t0 = time.perf_counter()
        hg, hp = numpy_form(h["baitID"], h["minOE"], h["maxOE"], h["p"], h["peak_baitID"], h["peak_oeID"], h["scores"], nc1, SCORE, PVCUT, MIND)
        line["host_numpy_ms"] = (time.perf_counter() - t0) * 1e3
        line["host_numpy_counts"] = [hg, hp]   # (rounding of delta at the cut-off aside, the device's counts)
    emit(line)
    del d, r
