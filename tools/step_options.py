"""bench.py's timed step (one wald_test call on synth.make(rows, samples)) with library options set — bench.py itself takes none —, for
kernel traces and counter passes of one route at a time and for whole-step A/Bs of two routes of ONE library:

    python tools/step_options.py ROWS SAMPLES STEPS WARMUP [option=value ...] [--runs R] [--dump DIR]
    rocprofv3 --kernel-trace --stats -d OUT --output-format csv -- python tools/step_options.py 2000000 8 10 2 sf_log_table=0

Prints one line per run: ms per step between two synchronisations, as bench.py measures it (the library CHICDIFF_HIP_LIB names, or the
tree's).  --dump DIR writes the last step's columns and scalars as DIR/<name>.npy for a comparison of two routes' outputs."""
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main():
    args = sys.argv[1:]
    runs, dump = 1, None
    if "--runs" in args:
        k = args.index("--runs"); runs = int(args[k + 1]); del args[k:k + 2]
    if "--dump" in args:
        k = args.index("--dump"); dump = args[k + 1]; del args[k:k + 2]
    n, S, steps, warmup = (int(x) for x in args[:4])
    import torch
    from chicdiff_amd import hip, synth
    ctx = hip.HipContext(0)
    for kv in args[4:]:
        name, v = kv.split("=")
        ctx.set_option(name, int(v))
    d = synth.make(n, S)
    dk = ctx.to_device(d["counts"], np.int32)
    dfm = ctx.to_device(d["nf"] * (d["mu"][:, None] / S), np.float64)
    want = ["baseMean", "dispersion", "log2FoldChange", "lfcSE", "stat", "pvalue", "maxCooks", "cooksArgmax"] + (["deviance", "betaIter"] if dump else [])
    outputs = {}
    for _ in range(warmup):
        ctx.wald_test(dk, dfm, d["group"], theta=0.5, want=want, outputs=outputs)
    for r in range(runs):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(steps):
            _, sc = ctx.wald_test(dk, dfm, d["group"], theta=0.5, want=want, outputs=outputs)
        torch.cuda.synchronize()
        print(f"{n} x {S} {' '.join(args[4:]) or '(defaults)'}: ms_per_step {(time.perf_counter() - t0) / steps * 1e3:.4f}", flush=True)
    if dump:
        os.makedirs(dump, exist_ok=True)
        for k, v in outputs.items():
            np.save(os.path.join(dump, k + ".npy"), v.cpu().numpy())
        np.save(os.path.join(dump, "sumDeviance.npy"), np.array([sc["sumDeviance"]]))
        np.save(os.path.join(dump, "sizeFactors.npy"), np.asarray(sc["sizeFactors"]))


main()
