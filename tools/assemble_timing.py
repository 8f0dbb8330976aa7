"""region_assemble against the three calls it replaces (count_join_multi -> fragment_background(only_fullmean) -> window_sums),
timed in ONE process, alternating, on the inputs of tests/assemble_inputs.py (the benchmark's end-to-end recipe).

    python3 tools/assemble_timing.py [--shapes 2000000x8,250000x8] [--reps 5] [--out FILE]

Two figures per path and repeat: ``events`` = device events around the whole path on the context's stream (what a caller waits
for, host gaps between the three calls included), ``kernels`` = the sum of the library's own per-stage device timers.  One JSON
line per shape: every repeat, the medians, min / max as the run-to-run spread, and the algorithmic bytes of both paths.
Under rocprofv3 (--kernel-trace --stats, or --pmc FETCH_SIZE WRITE_SIZE in a run of its own) use --reps 2: the kernels of
interest are region_assemble_kernel, count_join_multi_kernel, fragment_background_kernel and window_sums_kernel."""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
from assemble_inputs import assemble, background_args, make, three_calls  # noqa: E402
from chicdiff_amd import hip  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--shapes", default="2000000x8,250000x8")
ap.add_argument("--reps", type=int, default=5)
ap.add_argument("--out", default=None)
args = ap.parse_args()

ctx = hip.HipContext(0)
ctx.enable_timing(True)
lines = []
for shape in args.shapes.split(","):
    n, S = (int(x) for x in shape.split("x"))
    d = make(ctx, n, S, counts="synth")
    bg = background_args(d)
    call = dict(three_calls=lambda: three_calls(ctx, d["bait"], d["oe"], d["region_ptr"], d["tables"], bg),
                region_assemble=lambda: assemble(ctx, d["bait"], d["oe"], d["region_ptr"], d["tables"], bg))
    stages = dict(three_calls=("count_join_multi", "fragment_background", "window_sums"), region_assemble=("region_assemble",))

    def timed(name):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        kern = {}
        orig = ctx.kernel_times

        def collect():  # the library's timers hold the LAST call only: read them after each call of the path
            t = orig()
            for k in stages[name]:
                if k in t:
                    kern[k] = t[k][0]
            return t
        e0.record()
        if name == "three_calls":
            fragN = ctx.count_join_multi(d["bait"], d["oe"], d["tables"])
            collect()
            _, _, fragFM = ctx.fragment_background(d["bait"], d["oe"], *bg, only_fullmean=True)
            collect()
            out = ctx.window_sums(fragN, fragFM, d["region_ptr"])
            collect()
        else:
            out = call[name]()
            collect()
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1), kern, out

    for name in call:       # warm-up: code objects, the context's scratch, the allocator's blocks
        for _ in range(2):
            timed(name)
    res = {k: dict(events=[], kernels=[], stages=[]) for k in call}
    same = None
    for _ in range(args.reps):
        outs = {}
        for name in ("three_calls", "region_assemble"):   # alternating
            ms, kern, outs[name] = timed(name)
            res[name]["events"].append(ms)
            res[name]["kernels"].append(sum(kern.values()))
            res[name]["stages"].append(kern)
        if same is None:
            (Na, Fa), (Nr, Fr) = outs["region_assemble"], outs["three_calls"]
            nan = torch.isnan(Fr)
            same = bool(torch.equal(Na, Nr) and torch.equal(torch.isnan(Fa), nan) and torch.equal(Fa.view(torch.int64)[~nan], Fr.view(torch.int64)[~nan]))
        del outs
    nfrag, nkeys = d["nfrag"], sum(int(k.numel()) for k, _ in d["tables"])
    line = dict(shape=shape, n=n, S=S, nfrag=nfrag, nkeys_total=nkeys, reps=args.reps, outputs_bit_identical=same,
                bytes_three_calls=8 * nfrag + 12 * nkeys + 2 * 12 * S * nfrag + 12 * S * n,
                bytes_region_assemble=8 * nfrag + 12 * nkeys + 12 * S * n)
    for name, r in res.items():
        line[name] = dict(events_ms=[round(x, 4) for x in r["events"]], kernels_ms=[round(x, 4) for x in r["kernels"]],
                          events_median=round(float(np.median(r["events"])), 4), kernels_median=round(float(np.median(r["kernels"])), 4),
                          events_min_max=[round(min(r["events"]), 4), round(max(r["events"]), 4)],
                          kernels_min_max=[round(min(r["kernels"]), 4), round(max(r["kernels"]), 4)],
                          stages_median={k: round(float(np.median([s.get(k, 0.0) for s in r["stages"]])), 4) for k in stages[name]})
    lines.append(json.dumps(line))
    print(lines[-1], flush=True)
    del d, bg
    torch.cuda.empty_cache()
if args.out:
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")
