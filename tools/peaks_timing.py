"""readAndFilterPeakMatrix: the host reader (pandas) beside the device path (device=True) in one process, alternating, on synthetic
tab-separated peak matrices of 11 key columns and 8 score columns (makePeakMatrix layout, scores written with up to 15 digits).

    python3 tools/peaks_timing.py [--rows 200000,2000000] [--dev-reps 5] [--dir DIR] [--out profiles/r25_peaks_timing.jsonl]

Each file is read once untimed by each path (page cache warm, the context's buffers grown), then the two paths alternate; the host
path is repeated twice at up to 200 000 rows and once above (it takes tens of seconds there).  Whole readAndFilterPeakMatrix calls are
timed by the host clock with synchronised ends.  A second round of device reads runs with the library's event timer on.

One JSON line per file:
  rows, file_bytes, score_columns
  host_call_ms / dev_call_ms    whole calls (the device path's includes the header, the upload, the copy of the columns into torch
                                tensors, the filter, the gather of the kept rows and writing _filteredBaits.txt)
  dev_split_ms                  peaks_upload, peaks_mark (mark + quote pass), peaks_scan, peaks_parse, peaks_patch, peaks_filter
  kept, equal                   rows kept, and that the two paths keep the same rows with the same baitID / oeID (asserted)"""
import argparse
import json
import os
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

ap = argparse.ArgumentParser()
ap.add_argument("--rows", default="200000,2000000")
ap.add_argument("--dev-reps", type=int, default=5)
ap.add_argument("--dir", default=None)
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r25_peaks_timing.jsonl"))
args = ap.parse_args()

NAMES = ["A1", "A2", "A3", "A4", "B1", "B2", "B3", "B4"]
CHICAGO = {"A": {n: n for n in NAMES[:4]}, "B": {n: n for n in NAMES[4:]}}
KEYS = ["baitChr", "baitStart", "baitEnd", "baitID", "baitName", "oeChr", "oeStart", "oeEnd", "oeID", "oeName", "dist"]
BLOCK = 200_000


def block_text(n, seed=25):
    rng = np.random.default_rng(seed)
    bait = np.sort(rng.integers(1, 400_000, n))
    oe = bait + rng.integers(1, 300, n) * rng.choice([-1, 1], n)
    sc = rng.gamma(2.0, 3.0, (n, 8))
    na = rng.random((n, 8)) < 0.15
    trans = rng.random(n) < 0.03
    out = []
    for r in range(n):
        b, o = int(bait[r]), int(max(oe[r], 0))
        dist = "NA" if trans[r] else ("%.1f" % ((o - b) * 4000 + 0.5) if r % 2 else "%d" % ((o - b) * 4000))
        scores = ["NA" if na[r, j] else "%.15g" % sc[r, j] for j in range(8)]
        out.append("\t".join(["chr19", str(b * 4000), str(b * 4000 + 3999), str(b), f"gene{b}", "chr19", str(o * 4000), str(o * 4000 + 3999),
                              str(o), ".", dist] + scores))
    return ("\n".join(out) + "\n").encode()


def write_file(path, n):
    block = block_text(min(n, BLOCK))
    with open(path, "wb") as f:
        f.write(("\t".join(KEYS + NAMES) + "\n").encode())
        for _ in range(max(1, n // BLOCK)):
            f.write(block)
    return os.path.getsize(path)


import torch  # noqa: E402

from chicdiff_amd import hip, pipeline  # noqa: E402

ctx = hip.HipContext(0)
tmp = tempfile.mkdtemp(dir=args.dir)
for n in (int(r) for r in args.rows.split(",")):
    path = os.path.join(tmp, f"peaks_{n}.txt")
    nbytes = write_file(path, n)
    rows = max(1, n // BLOCK) * min(n, BLOCK)
    line = dict(rows=rows, file_bytes=nbytes, score_columns=len(NAMES), host_cpus=len(os.sched_getaffinity(0)))

    def timed(device):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        x = pipeline.readAndFilterPeakMatrix(path, NAMES, CHICAGO, list(CHICAGO), 5.0, outprefix=os.path.join(tmp, "d" if device else "h"),
                                             ctx=ctx if device else None, device=device)
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3, x

    h0, hx = timed(False)                  # untimed: page cache, staging areas, device buffers
    _, dx = timed(True)
    assert np.array_equal(dx["baitID"].cpu().numpy(), hx["baitID"].to_numpy(np.int32))
    assert np.array_equal(dx["oeID"].cpu().numpy(), hx["oeID"].to_numpy(np.int32))
    assert np.array_equal(dx["dist"].cpu().numpy(), hx["dist"].to_numpy(np.float64))
    assert open(os.path.join(tmp, "d_filteredBaits.txt"), "rb").read() == open(os.path.join(tmp, "h_filteredBaits.txt"), "rb").read()
    line.update(kept=len(hx), equal=True)
    del hx, dx
    host_reps = 2 if rows <= 200_000 else 1
    host_ms, dev_ms = [], []
    for k in range(args.dev_reps):
        if k < host_reps:
            host_ms.append(timed(False)[0])
        dev_ms.append(timed(True)[0])
    line.update(host_call_ms=host_ms, host_call_median_ms=float(np.median(host_ms)), host_first_untimed_call_ms=h0, dev_call_ms=dev_ms,
                dev_call_median_ms=float(np.median(dev_ms)), dev_call_range_ms=[min(dev_ms), max(dev_ms)])
    ctx.enable_timing(True)
    split = {}
    for _ in range(args.dev_reps):
        pk = ctx.read_peaks(path, NAMES)
        for k, (ms, _) in ctx.kernel_times().items():
            split.setdefault(k, []).append(ms)
        ctx.filter_peaks(pk, 5.0, [0] * 4 + [1] * 4, True)
        for k, (ms, _) in ctx.kernel_times().items():
            split.setdefault(k, []).append(ms)
        del pk
    ctx.enable_timing(False)
    line["dev_split_ms"] = split
    line["dev_split_median_ms"] = {k: float(np.median(v)) for k, v in split.items()}
    print(json.dumps(line), flush=True)
    with open(args.out, "a") as f:
        f.write(json.dumps(line) + "\n")
    os.remove(path)
for f in os.listdir(tmp):
    os.remove(os.path.join(tmp, f))
os.rmdir(tmp)
ctx.close()
