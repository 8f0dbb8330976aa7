"""readAndFilterPeakMatrix on SEVERAL peak files: the host reader (pandas: read_csv per file, outer merge) beside the device path
(device=True, device_merge=True) in one process, alternating, on synthetic tab-separated peak matrices of 11 key columns and 4 score
columns each (makePeakMatrix layout, scores written with up to 15 digits, 15 % NA, 3 % trans rows, rows in random order).

    python3 tools/peaks_merge_timing.py [--rows 1000000,2000000] [--dev-reps 5] [--dir DIR] [--out profiles/r28_peaks_merge_timing.jsonl]

Two files of --rows rows each share half of their keys.  Each set is read once untimed by each path (page cache warm, the context's
buffers grown), then the two paths alternate; the host path is timed once (it takes tens of seconds per file).  Whole
readAndFilterPeakMatrix calls are timed by the host clock with synchronised ends.  A second round of device calls runs piece by piece
with the library's event timer on.

One JSON line per size:
  rows_per_file, files, file_bytes, score_columns_per_file, merged_rows
  host_call_ms / dev_call_ms    whole calls (the device path's includes the headers, the uploads, the copies of the columns into torch
                                tensors, the keys, the merge, the filter, the gather of the kept rows and writing _filteredBaits.txt)
  dev_split_ms                  per file: peaks_upload, peaks_mark, peaks_scan, peaks_parse, peaks_textkeys; then peaks_merge_sort,
                                peaks_merge_heads (heads + scan), peaks_merge_write, peaks_filter
  kept, equal                   rows kept, and that the two paths keep the same rows with the same baitID / oeID / dist and write
                                the same _filteredBaits.txt (asserted)"""
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
ap.add_argument("--rows", default="1000000,2000000")
ap.add_argument("--dev-reps", type=int, default=5)
ap.add_argument("--dir", default=None)
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r28_peaks_merge_timing.jsonl"))
args = ap.parse_args()

NAMES = [["A1", "A2", "B1", "B2"], ["A3", "A4", "B3", "B4"]]
TARGETS = NAMES[0] + NAMES[1]
CHICAGO = {"A": {n: n for n in TARGETS if n[0] == "A"}, "B": {n: n for n in TARGETS if n[0] == "B"}}
KEYS = ["baitChr", "baitStart", "baitEnd", "baitID", "baitName", "oeChr", "oeStart", "oeEnd", "oeID", "oeName", "dist"]


def write_set(tmp, n, seed=28):
    """Two files of n rows over 3 n / 2 distinct keys: file 0 holds the first n, file 1 the last n, each in random order."""
    import pandas as pd
    rng = np.random.default_rng(seed)
    u = 3 * n // 2
    i = np.arange(u, dtype=np.int64)
    bait = i // 16 + 1000                                                          # 16 other ends per bait, on both sides
    oe = bait + (i % 8 + 2) * np.where(i % 16 < 8, 1, -1)
    trans = rng.random(u) < 0.03
    dist = np.where(trans, np.nan, (oe - bait) * 4000 + np.where(i % 2 == 1, 0.5, 0.0))
    chrom = np.where(bait % 3 == 0, "chr19", np.where(bait % 3 == 1, "chr2", "chrX"))
    keys = pd.DataFrame({"baitChr": chrom, "baitStart": bait * 4000, "baitEnd": bait * 4000 + 3999, "baitID": bait,
                         "baitName": ["gene%d" % b for b in bait], "oeChr": np.where(trans, "chr1", chrom), "oeStart": oe * 4000,
                         "oeEnd": oe * 4000 + 3999, "oeID": oe, "oeName": ".", "dist": dist})
    paths = []
    for f, (lo, hi) in enumerate(((0, n), (u - n, u))):
        x = keys.iloc[lo:hi].copy()
        sc = rng.gamma(2.0, 3.0, (n, 4))
        sc[rng.random((n, 4)) < 0.15] = np.nan
        for j, name in enumerate(NAMES[f]):
            x[name] = sc[:, j]
        x = x.iloc[rng.permutation(n)]
        paths.append(os.path.join(tmp, f"peaks_{n}_{f}.txt"))
        x.to_csv(paths[f], sep="\t", index=False, na_rep="NA", float_format="%.15g")
    return paths


import torch  # noqa: E402

from chicdiff_amd import hip, pipeline  # noqa: E402

ctx = hip.HipContext(0)
tmp = tempfile.mkdtemp(dir=args.dir)
for n in (int(r) for r in args.rows.split(",")):
    paths = write_set(tmp, n)
    line = dict(rows_per_file=n, files=len(paths), file_bytes=[os.path.getsize(p) for p in paths], score_columns_per_file=4,
                host_cpus=len(os.sched_getaffinity(0)))

    def timed(device):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        x = pipeline.readAndFilterPeakMatrix(paths, TARGETS, CHICAGO, list(CHICAGO), 5.0, outprefix=os.path.join(tmp, "d" if device else "h"),
                                             ctx=ctx if device else None, device=device, device_merge=device)
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3, x

    h0, hx = timed(False)                  # untimed: page cache, staging areas, device buffers
    _, dx = timed(True)
    assert dx.frame is None, "the device path declined"
    assert np.array_equal(dx["baitID"].cpu().numpy(), hx["baitID"].to_numpy(np.int32))
    assert np.array_equal(dx["oeID"].cpu().numpy(), hx["oeID"].to_numpy(np.int32))
    assert np.array_equal(dx["dist"].cpu().numpy(), hx["dist"].to_numpy(np.float64))
    assert open(os.path.join(tmp, "d_filteredBaits.txt"), "rb").read() == open(os.path.join(tmp, "h_filteredBaits.txt"), "rb").read()
    line.update(kept=len(hx), equal=True)
    del hx, dx
    host_ms, dev_ms = [], []
    for k in range(args.dev_reps):
        if k < 1:
            host_ms.append(timed(False)[0])
        dev_ms.append(timed(True)[0])
    line.update(host_call_ms=host_ms, host_call_median_ms=float(np.median(host_ms)), host_first_untimed_call_ms=h0, dev_call_ms=dev_ms,
                dev_call_median_ms=float(np.median(dev_ms)), dev_call_range_ms=[min(dev_ms), max(dev_ms)])
    ctx.enable_timing(True)
    split = {}

    def note(prefix=""):
        for k, (ms, _) in ctx.kernel_times().items():
            split.setdefault(prefix + k, []).append(ms)
    for _ in range(args.dev_reps):
        pks = []
        for f, p in enumerate(paths):
            pk = ctx.read_peaks(p, NAMES[f])
            note(f"file{f}.")
            ctx.peaks_text_keys(pk)
            note(f"file{f}.")
            pks.append(pk)
        m = ctx.merge_peaks(pks)
        note()
        line["merged_rows"] = m.n
        cond = [0 if c[0] == "A" else 1 for c in m.score_names]
        ctx.filter_peaks(m, 5.0, cond, True)
        note()
        del pks, m
    ctx.enable_timing(False)
    line["dev_split_ms"] = split
    line["dev_split_median_ms"] = {k: float(np.median(v)) for k, v in split.items()}
    print(json.dumps(line), flush=True)
    with open(args.out, "a") as f:
        f.write(json.dumps(line) + "\n")
    for p in paths:
        os.remove(p)
for f in os.listdir(tmp):
    os.remove(os.path.join(tmp, f))
os.rmdir(tmp)
ctx.close()
