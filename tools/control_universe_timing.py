"""getControlRegionUniverse: the host draws (``rng=``: RU copied to the host, pandas groupby, np.unique, numpy draws, pandas sort)
beside the seeded device draws (``seed=`` -> chicdiff_hip_control_draws_dev), in one process and alternating.

    python3 tools/control_universe_timing.py [--peaks 250000,2000000] [--reps 7] [--out FILE] [--device-only]
    python3 tools/control_universe_timing.py --ingest-stats KERNEL_STATS.csv --out FILE

Geometry: the benchmark's map (bench.py: 840 000 fragments, a chromosome per 35 000 IDs), written as the rmap / baitmap files the
stage reads; 22 000 baits; peaks 2 .. 59 fragments from their bait, turned to the other side where the window would leave the
chromosome; RUexpand = 5.  The test universe comes from the device expansion and stays on the device.

One JSON line per size: for each path the whole call (host clock around a call that ends synchronised) and its parts —
  read_ms     reading the restriction map (both paths read it; a part of neither's draws)
  expand_ms   the shared expansion of the drawn pairs (post.getRegionUniverse)
  front_ms    whole - read - expand: everything in front of the expansion — what this comparison is about
  kernels_ms  (device) the library's own event timers around the contact pass, the draws, the sort and the unpack
``--ingest-stats``: the rows of a ``rocprofv3 --kernel-trace --stats`` run of this tool (``--device-only``), one JSON line per kernel."""
import argparse
import csv
import json
import os
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

ap = argparse.ArgumentParser()
ap.add_argument("--peaks", default="250000,2000000")
ap.add_argument("--reps", type=int, default=7)
ap.add_argument("--out", default=None)
ap.add_argument("--device-only", action="store_true")
ap.add_argument("--ingest-stats", default=None)
args = ap.parse_args()


def emit(line):
    print(json.dumps(line), flush=True)
    if args.out:
        with open(args.out, "a") as f:
            f.write(json.dumps(line) + "\n")


if args.ingest_stats:
    with open(args.ingest_stats, newline="") as f:
        for row in csv.DictReader(f):
            emit(dict(kind="kernel_stats", source="rocprofv3 --kernel-trace --stats, device path only", **row))
    sys.exit(0)

import torch  # noqa: E402

from chicdiff_amd import hip, pipeline, post, settings as st  # noqa: E402

MAXFRAG, PER_CHR, NBAITS = 840000, 35000, 22000
tmp = tempfile.mkdtemp(prefix="control_universe_timing_")
ids = np.arange(1, MAXFRAG + 1, dtype=np.int64)
chrom = np.char.add("chr", (ids // PER_CHR).astype(str))
rng0 = np.random.default_rng(17)
bait_rows = np.sort(rng0.choice(len(ids), NBAITS, replace=False))
rmapfile, baitmapfile = os.path.join(tmp, "synth.rmap"), os.path.join(tmp, "synth.baitmap")
with open(rmapfile, "w") as f:
    f.write("".join(f'"{c}" {4000 * i - 3999} {4000 * i} {i}\n' for c, i in zip(chrom, ids)))
with open(baitmapfile, "w") as f:
    f.write("".join(f'"{chrom[r]}" {4000 * ids[r] - 3999} {4000 * ids[r]} {ids[r]} "gene{ids[r]}"\n' for r in bait_rows))
s = st.defaultChicdiffSettings()
s.update(rmapfile=rmapfile, baitmapfile=baitmapfile, outprefix=os.path.join(tmp, "t"), RUexpand=5)

ctx = hip.HipContext(0)
ctx.enable_timing(True)
parts = {}


def timed(name, fn):
    def wrapper(*a, **k):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        r = fn(*a, **k)
        torch.cuda.synchronize()
        parts[name] = parts.get(name, 0.0) + (time.perf_counter() - t0) * 1e3
        return r
    return wrapper


pipeline._read_rmap = timed("read", pipeline._read_rmap)
post.getRegionUniverse = timed("expand", post.getRegionUniverse)

for n in (int(p) for p in args.peaks.split(",")):
    g = torch.Generator(device=ctx.device)
    g.manual_seed(1)
    pb = torch.from_numpy(ids[bait_rows]).to(ctx.device)[torch.randint(0, NBAITS, (n,), device=ctx.device, generator=g)].to(torch.int32)
    dd = torch.randint(2, 60, (n,), dtype=torch.int32, device=ctx.device, generator=g)
    off_chr = ((pb + dd + 5) // PER_CHR != pb // PER_CHR) | (pb + dd + 5 > MAXFRAG)
    po = pb + torch.where(off_chr, -dd, dd)
    parts.clear()
    RU = pipeline.RegionUniverse(post.getRegionUniverse(ctx, pb, po, 5, chrom, ids))
    line = dict(kind="timing", peaks=n, RUexpand=5, ru_rows=int(RU["baitID"].numel()), fragments=MAXFRAG, baits=NBAITS, reps=args.reps,
                host_cpus=len(os.sched_getaffinity(0)))
    acc = {"host": [], "device": []}
    for rep in range(args.reps + 1):                                             # the first repeat warms both paths up
        for path in (("device",) if args.device_only else ("host", "device")):   # alternating
            parts.clear()
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            if path == "host":
                ruc = pipeline.getControlRegionUniverse(s, RU, ctx, rng=np.random.default_rng(rep))
            else:
                ruc = pipeline.getControlRegionUniverse(s, RU, ctx, seed=rep)
            torch.cuda.synchronize()
            whole = (time.perf_counter() - t0) * 1e3
            rec = dict(whole_ms=whole, read_ms=parts.get("read", 0.0), expand_ms=parts.get("expand", 0.0))
            rec["front_ms"] = whole - rec["read_ms"] - rec["expand_ms"]
            if path == "device":
                rec["kernels_ms"] = ctx.last_control_draws_ms
            rec["control_regions"] = int(ruc["region_ptr"].numel() - 1)
            if rep:
                acc[path].append(rec)
            del ruc
    for path, recs in acc.items():
        if recs:
            line[path] = {k: [r[k] for r in recs] for k in recs[0]}
            line[path + "_median"] = {k: float(np.median([r[k] for r in recs])) for k in recs[0]}
    if acc["host"]:
        line["whole_speedup"] = line["host_median"]["whole_ms"] / line["device_median"]["whole_ms"]
        line["front_speedup"] = line["host_median"]["front_ms"] / line["device_median"]["front_ms"]
    emit(line)
    del RU, pb, po
