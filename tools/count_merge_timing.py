"""The branch without chinput files for TWO region sets (test and control), three ways, timed in ONE process, alternating:

  inner           per set: count_join_inner -> fragment_background(only_fullmean) -> window_sums          (the default path)
  merge_assemble  merge_count_tables once, then per set: region_assemble on the merged tables
  merge_multi     merge_count_tables once, then per set: count_join_multi -> fragment_background -> window_sums

    python3 tools/count_merge_timing.py [--shapes 250000x8,2000000x8] [--reps 7] [--drop 0.1] [--out FILE]

Inputs: tests/assemble_inputs.py (the benchmark's end-to-end recipe); the second region set is the universe of a second seed; every
replicate's table loses a seeded share ``--drop`` of its pairs, so that the inner join differs from the left join.  The three results
are asserted equal (bit for bit) before anything is timed.  Two figures per path and repeat, after one warm call: ``events`` = device
events around the whole path on the context's stream (host gaps and the merge's one host stop included), ``kernels`` = the sum of the
library's own per-stage device timers.  One JSON line per shape: every repeat, medians, min / max as the run-to-run spread."""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
from assemble_inputs import background_args, make  # noqa: E402
from chicdiff_amd import hip  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--shapes", default="250000x8,2000000x8")
ap.add_argument("--reps", type=int, default=7)
ap.add_argument("--drop", type=float, default=0.1)
ap.add_argument("--out", default=None)
args = ap.parse_args()

ctx = hip.HipContext(0)
ctx.enable_timing(True)
PATHS = ("inner", "merge_assemble", "merge_multi")
lines = []
for shape in args.shapes.split(","):
    n, S = (int(x) for x in shape.split("x"))
    d = make(ctx, n, S, counts="synth")
    bg = background_args(d)
    other = make(ctx, n, S, seed=8, counts="device", table_share=0.01)
    sets = [(d["bait"], d["oe"], d["region_ptr"]), (other["bait"], other["oe"], other["region_ptr"])]
    del other
    g = torch.Generator(device=ctx.device)
    g.manual_seed(99)
    tables = []
    for ks, vs in d["tables"]:
        keep = torch.rand(ks.numel(), device=ctx.device, generator=g) >= args.drop
        tables.append((ks[keep].contiguous(), vs[keep].contiguous()))
    d["tables"] = None

    def run(name):
        """-> (ms by events, {stage: ms by the library's timers, summed over the path's calls}, [(N, FullMean) per set])"""
        kern = {}

        def collect():  # the library's timers hold the LAST call only
            for k, t in ctx.kernel_times().items():
                if t[1] > 0:
                    kern[k] = kern.get(k, 0.0) + t[0]
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        outs = []
        e0.record()
        use = tables
        if name != "inner":
            use = ctx.merge_count_tables(tables)
            collect()
        for bait, oe, ptr in sets:
            if name == "merge_assemble":
                outs.append(ctx.region_assemble(bait, oe, ptr, use, *bg))
                collect()
                continue
            fragN = ctx.count_join_inner(bait, oe, use) if name == "inner" else ctx.count_join_multi(bait, oe, use)
            collect()
            _, _, fragFM = ctx.fragment_background(bait, oe, *bg, only_fullmean=True)
            collect()
            outs.append(ctx.window_sums(fragN, fragFM, ptr))
            collect()
            del fragN, fragFM
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1), kern, outs

    ref = run("inner")[2]                                              # the warm call of every path, and the comparison
    assert all(bool((N > 0).any()) for N, _ in ref)
    left = ctx.count_join_multi(*sets[0][:2], tables)
    assert not torch.equal(left, ctx.count_join_inner(*sets[0][:2], tables)), "the inner join must differ from the left join"
    del left
    for name in PATHS[1:]:
        for (N, F), (Nr, Fr) in zip(run(name)[2], ref):
            nan = torch.isnan(Fr)
            assert torch.equal(N, Nr) and torch.equal(torch.isnan(F), nan) and torch.equal(F.view(torch.int64)[~nan], Fr.view(torch.int64)[~nan]), name
    del ref
    res = {k: dict(events=[], kernels=[], stages=[]) for k in PATHS}
    for _ in range(args.reps):
        for name in PATHS:                                             # alternating
            ms, kern, _ = run(name)
            res[name]["events"].append(ms)
            res[name]["kernels"].append(sum(kern.values()))
            res[name]["stages"].append(kern)
    merged_keys = int(ctx.merge_count_tables(tables)[0][0].numel())
    line = dict(shape=shape, n=n, S=S, region_sets=len(sets), nfrag=[int(b.numel()) for b, _, _ in sets],
                nkeys=[int(k.numel()) for k, _ in tables], merged_keys=merged_keys, drop=args.drop, reps=args.reps, outputs_bit_identical=True)
    for name, r in res.items():
        names = sorted({k for s in r["stages"] for k in s})
        line[name] = dict(events_ms=[round(x, 4) for x in r["events"]], kernels_ms=[round(x, 4) for x in r["kernels"]],
                          events_median=round(float(np.median(r["events"])), 4), kernels_median=round(float(np.median(r["kernels"])), 4),
                          events_min_max=[round(min(r["events"]), 4), round(max(r["events"]), 4)],
                          kernels_min_max=[round(min(r["kernels"]), 4), round(max(r["kernels"]), 4)],
                          stages_median={k: round(float(np.median([s.get(k, 0.0) for s in r["stages"]])), 4) for k in names})
    lines.append(json.dumps(line))
    print(lines[-1], flush=True)
    del d, bg, sets, tables
    torch.cuda.empty_cache()
if args.out:
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")
