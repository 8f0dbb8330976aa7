"""countput: the host twin (pipeline._countput, a pandas groupby) beside the device path (pipeline.countput_dev ->
chicdiff_hip_countput_dev) in one process, alternating, at the size of real Chicago tables.

    python3 tools/countput_timing.py [--rows 250000,2000000] [--replicates 4] [--reps 7] [--host-reps 3] [--out FILE] [--no-host]

Geometry: a human-sized restriction map (840 000 fragments, id_min = 1, 2 % of the IDs missing), 22 000 baits, every row an other end
within 3 000 fragments of its bait; two conditions of ``replicates`` replicates; the replicates of a condition draw their rows from
one universe of 1.75 x rows pairs, so most groups hold rows of several replicates.  10 % of Bmean, score and distSign are NaN.  Every
replicate is shuffled (the twin's and the device's work do not depend on the row order beyond the order of the output).

One JSON line per size:
  host_twin_ms      ``host-reps`` runs of pipeline._countput on this host's CPU
  dev_kernels_ms    (a) ``reps`` runs of HipContext.countput on columns already on the device: the library's own event timer around
                    key pass, sort, heads, scan and reduce, summed over the two conditions
  dev_call_ms       (b) the same calls with the upload of the six columns per replicate in front — host clock, ends synchronised
  dev_frame_ms      (c) pipeline.countput_dev: uploads, calls, read-back of the six columns and the DataFrame
  groups            rows of the frame; the device's frame equals the twin's bit for bit (asserted when the host runs)"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

ap = argparse.ArgumentParser()
ap.add_argument("--rows", default="250000,2000000")
ap.add_argument("--replicates", type=int, default=4)
ap.add_argument("--reps", type=int, default=7)
ap.add_argument("--host-reps", type=int, default=3)
ap.add_argument("--out", default=None)
ap.add_argument("--no-host", action="store_true")
args = ap.parse_args()

NID, ID_MIN, NBAITS = 840000, 1, 22000


def emit(line):
    print(json.dumps(line), flush=True)
    if args.out:
        with open(args.out, "a") as f:
            f.write(json.dumps(line) + "\n")


def the_map(seed=20):
    import pandas as pd
    rng = np.random.default_rng(seed)
    start = 4000 * np.arange(NID, dtype=np.int64) + rng.integers(0, 500, NID)
    end = start + rng.integers(200, 3500, NID)
    chr_codes = (np.arange(NID) // 40000).astype(np.int32)
    chr_codes[rng.random(NID) < 0.02] = -1
    on = chr_codes >= 0
    rmap = pd.DataFrame({"OEchr": chr_codes[on].astype(str), "OEstart": start[on], "OEend": end[on],
                         "otherEndID": (ID_MIN + np.arange(NID, dtype=np.int64))[on]})
    return np.where(on, start + end, 0), chr_codes, rmap


def make(n, R, seed):
    import pandas as pd
    rng = np.random.default_rng(seed)
    baits = np.sort(rng.choice(np.arange(ID_MIN + 3000, ID_MIN + NID - 3000), NBAITS, replace=False))
    b = baits[rng.integers(0, NBAITS, 2 * n)]
    o = b + rng.integers(1, 3001, 2 * n) * rng.choice([-1, 1], 2 * n)
    key = np.unique((b.astype(np.int64) << 32) | o)
    rng.shuffle(key)
    key = key[: n + 3 * n // 4]
    xs = []
    for r in range(R):
        k = rng.choice(key, min(n, len(key)), replace=False)
        m = len(k)
        val = lambda v: np.where(rng.random(m) < 0.1, np.nan, v)
        xs.append(pd.DataFrame({"baitID": (k >> 32).astype(np.int32), "otherEndID": (k & 0xFFFFFFFF).astype(np.int32),
                                "N": rng.integers(1, 400, m).astype(np.int32), "Bmean": val(np.exp(rng.normal(0, 1.0, m))),
                                "score": val(rng.gamma(2.0, 2.0, m)), "distSign": val(np.rint(rng.normal(0, 1e5, m)))}))
    return xs


import torch  # noqa: E402

from chicdiff_amd import hip, pipeline  # noqa: E402

ctx = hip.HipContext(0)
ctx.enable_timing(True)
dev = lambda a, t: torch.from_numpy(np.ascontiguousarray(a, dtype=t)).to(ctx.device)
midsum, chr_codes, rmap = the_map()
d_midsum, d_chr = dev(midsum, np.int64), dev(chr_codes, np.int32)
R = args.replicates
KINDS = (("baitID", np.int32), ("otherEndID", np.int32), ("N", np.int32), ("Bmean", np.float64), ("score", np.float64), ("distSign", np.float64))
upload = lambda xs_: [tuple(dev(x[c].to_numpy(), t) for c, t in KINDS) for x in xs_]

for n in (int(r) for r in args.rows.split(",")):
    xs = make(n, R, 1) + make(n, R, 2)
    conditions = ["A"] * R + ["B"] * R
    line = dict(rows_per_replicate=n, replicates=R, conditions=2, rows=sum(len(x) for x in xs), nid=NID, reps=args.reps)
    host_ms, kern_ms, call_ms, frame_ms = [], [], [], []
    want = got = None
    nhost = 0 if args.no_host else args.host_reps
    for rep in range(args.reps + 2):                                  # two warm-up rounds on the device side
        if rep >= 2 and rep - 2 < nhost:
            print(f"# {n} rows per replicate: host twin, run {rep - 1}", file=sys.stderr, flush=True)
            t0 = time.perf_counter()
            want = pipeline._countput(xs, conditions, rmap)
            host_ms.append((time.perf_counter() - t0) * 1e3)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        k_ms = 0.0
        for cond in ("A", "B"):
            cols = upload([x for x, c in zip(xs, conditions) if c == cond])
            ctx.countput(cols, ID_MIN, d_midsum, d_chr)
            k_ms += ctx.last_countput_ms
            del cols
        torch.cuda.synchronize()
        t1 = time.perf_counter()
        got = pipeline.countput_dev(xs, conditions, ctx, ID_MIN, d_midsum, d_chr)
        t2 = time.perf_counter()
        if rep >= 2:
            kern_ms.append(k_ms)
            call_ms.append((t1 - t0) * 1e3)
            frame_ms.append((t2 - t1) * 1e3)
    line.update(groups=len(got), dev_kernels_ms=kern_ms, dev_kernels_median_ms=float(np.median(kern_ms)), dev_call_ms=call_ms,
                dev_call_median_ms=float(np.median(call_ms)), dev_frame_ms=frame_ms, dev_frame_median_ms=float(np.median(frame_ms)))
    if want is not None:
        line.update(host_twin_ms=host_ms, host_twin_median_ms=float(np.median(host_ms)), host_cpus=len(os.sched_getaffinity(0)))
        assert list(got.columns) == list(want.columns) and len(got) == len(want)
        for k in got.columns:                                         # ... and the device's frame is the twin's
            a, b = got[k].to_numpy(), want[k].to_numpy()
            if a.dtype == np.float64:
                assert np.array_equal(np.isnan(a), np.isnan(b)) and np.array_equal(a[~np.isnan(a)].view(np.int64), b[~np.isnan(b)].view(np.int64)), k
            else:
                assert a.dtype == b.dtype and np.array_equal(a, b), k
        line["equal_to_host_twin"] = True
    emit(line)
    del xs, got, want
