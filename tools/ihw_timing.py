"""Training the IHW weights on the device (HipContext.ihw_train -> chicdiff_hip_ihw_train_dev), timed by the library's own event timers.

    python3 tools/ihw_timing.py [--rows 250000,2000000] [--bins 40] [--folds 5] [--reps 7] [--out FILE] [--twin-rows 0]

Data: a covariate like |avDist| (log-uniform), p-values uniform with a share of signal that falls with the covariate (tests/ihw_inputs.py).
One JSON line per size: the whole call (host clock around a call that ends synchronised) and the stages of the library's timers —
  ihw_rank    keys, the covariate sort, group and fold
  ihw_sorts   the sorts by p and by group, (p, fold) gathered in that order
  ihw_hulls   chunk fold histogram, scan, chunk hulls
  ihw_merge   the merge levels, segment counts and offsets
  ihw_sweep   segments, the sort by slope, the sweep
  host_ms     whole - the stages: the two host stops, allocation of the outputs, Python
``--twin-rows N``: also the numpy / Python twin's time at N rows (tests/ihw_twin.py), labelled as such — there is no R and no IHW
package here to compare with."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

ap = argparse.ArgumentParser()
ap.add_argument("--rows", default="250000,2000000")
ap.add_argument("--bins", type=int, default=40)
ap.add_argument("--folds", type=int, default=5)
ap.add_argument("--reps", type=int, default=7)
ap.add_argument("--out", default=None)
ap.add_argument("--twin-rows", type=int, default=0)
args = ap.parse_args()

import torch  # noqa: E402

import ihw_inputs  # noqa: E402
from chicdiff_amd import hip  # noqa: E402


def emit(line):
    print(json.dumps(line), flush=True)
    if args.out:
        with open(args.out, "a") as f:
            f.write(json.dumps(line) + "\n")


ctx = hip.HipContext(0)
ctx.enable_timing(True)
STAGES = ("ihw_rank", "ihw_sorts", "ihw_hulls", "ihw_merge", "ihw_sweep")
for n in (int(x) for x in args.rows.split(",")):
    p, cov = ihw_inputs.signal(n, 1)
    dp, dc = torch.from_numpy(p).to(ctx.device), torch.from_numpy(cov).to(ctx.device)
    recs = []
    for rep in range(args.reps + 1):   # the first call warms up (scratch allocation, code load)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        r = ctx.ihw_train(dp, dc, alpha=0.05, nbins=args.bins, nfolds=args.folds, seed=rep)
        torch.cuda.synchronize()
        whole = (time.perf_counter() - t0) * 1e3
        rec = dict(whole_ms=whole, **{k: ctx.last_ihw_train_ms.get(k, 0.0) for k in STAGES})
        rec["host_ms"] = whole - sum(rec[k] for k in STAGES)
        rec["segments"] = int(r["nseg"].sum())
        if rep:
            recs.append(rec)
    line = dict(kind="timing", rows=n, nbins=args.bins, nfolds=args.folds, reps=args.reps, chunk_len=r["chunk_len"],
                runs={k: [x[k] for x in recs] for k in recs[0]}, median={k: float(np.median([x[k] for x in recs])) for k in recs[0]})
    emit(line)
if args.twin_rows:
    import ihw_twin
    p, cov = ihw_inputs.signal(args.twin_rows, 1)
    t0 = time.perf_counter()
    ihw_twin.train(p, cov, 0.05, args.bins, args.folds, 1)
    emit(dict(kind="twin", note="tests/ihw_twin.py (numpy + Python integers) on the host: not the IHW package",
              rows=args.twin_rows, nbins=args.bins, nfolds=args.folds, seconds=time.perf_counter() - t0, host_cpus=len(os.sched_getaffinity(0))))
