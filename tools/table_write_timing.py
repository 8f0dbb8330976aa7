"""Writing a countput-shaped table: pandas' DataFrame.to_csv beside HipContext.write_table (chicdiff_hip_table_write_dev) in one process,
alternating, with the two files asserted equal.

    python3 tools/table_write_timing.py [--rows 1000000,7000000] [--reps 5] [--out profiles/r30_table_write_timing.jsonl] [--dir DIR]

The table: two int32 ID columns, four float64 columns (a mean of counts, a gamma draw, a score with 10 % NaN, a midpoint) and one
constant ``condition`` column — what ``_countput.csv`` holds.  Per size: one untimed warm call of each path, then ``reps`` timed device
calls and one timed host call.  The device columns are on the device before the clock starts (as they are behind ``countput_dev``);
the frame is in host memory before the host's clock starts.

One JSON line per size:
  rows, text_bytes          the table and the size of its file (header included)
  host_to_csv_ms            the timed ``to_csv(index=False)`` on this host's CPU (one thread: pandas formats row by row)
  dev_call_ms               the timed ``write_table`` calls, host clock, file closed when the call returns
  dev_len_ms / dev_scan_ms / dev_write_ms / dev_download_ms
                            the same calls split by the library's event timer: length pass, scan of the tile totals, write pass,
                            download through the pinned halves with the file writes between the DMAs
  ratio                     host_to_csv_ms / median(dev_call_ms)
  equal                     the two files compared byte for byte (asserted)"""
import argparse
import filecmp
import json
import os
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

ap = argparse.ArgumentParser()
ap.add_argument("--rows", default="1000000,7000000")
ap.add_argument("--reps", type=int, default=5)
ap.add_argument("--out", default=None)
ap.add_argument("--dir", default=None, help="where the two files are written (default: a temporary directory)")
args = ap.parse_args()

HEADER = ["baitID", "otherEndID", "Nav", "Bav", "score", "oeID_mid", "condition"]


def emit(line):
    print(json.dumps(line), flush=True)
    if args.out:
        with open(args.out, "a") as f:
            f.write(json.dumps(line) + "\n")


def make(n, seed=30):
    import pandas as pd
    rng = np.random.default_rng(seed)
    score = rng.gamma(2.0, 3.0, size=n)
    score[rng.random(n) < 0.1] = np.nan
    return pd.DataFrame({"baitID": rng.integers(1, 840000, size=n).astype(np.int32), "otherEndID": rng.integers(1, 840000, size=n).astype(np.int32),
                         "Nav": rng.integers(0, 400, size=n) / rng.integers(1, 5, size=n).astype(np.float64), "Bav": rng.gamma(1.5, 2.0, size=n),
                         "score": score, "oeID_mid": rng.integers(1, 10 ** 8, size=n).astype(np.float64) / 2.0, "condition": "treated"})


import torch  # noqa: E402

from chicdiff_amd import hip  # noqa: E402

ctx = hip.HipContext(0)
ctx.enable_timing(True)
tmp = args.dir or tempfile.mkdtemp(prefix="table_write_timing_")
host_path, dev_path = os.path.join(tmp, "host.csv"), os.path.join(tmp, "dev.csv")

for n in (int(r) for r in args.rows.split(",")):
    frame = make(n)
    cols = [torch.from_numpy(frame[c].to_numpy()).to(ctx.device) for c in HEADER[:-1]] + [(None, ["treated"])]
    torch.cuda.synchronize()
    note = lambda what: print(f"# {n} rows: {what}", file=sys.stderr, flush=True)
    note("warm device call")
    ctx.write_table(dev_path, cols, HEADER, n=n)
    note("warm host call")
    frame.to_csv(host_path, index=False)
    assert filecmp.cmp(host_path, dev_path, shallow=False), "the device's file differs from to_csv's"
    call_ms, parts = [], {k: [] for k in ("len", "scan", "write", "download")}
    host_ms = None
    for rep in range(args.reps):
        note(f"device call {rep + 1}")
        os.remove(dev_path)
        t0 = time.perf_counter()
        ctx.write_table(dev_path, cols, HEADER, n=n)
        call_ms.append((time.perf_counter() - t0) * 1e3)
        for k in parts:
            parts[k].append(ctx.last_table_write_ms.get(k, 0.0))
        if rep == args.reps // 2:                                     # the host's run sits between the device's
            note("host call")
            os.remove(host_path)
            t0 = time.perf_counter()
            frame.to_csv(host_path, index=False)
            host_ms = (time.perf_counter() - t0) * 1e3
    assert filecmp.cmp(host_path, dev_path, shallow=False), "the device's file differs from to_csv's"
    line = dict(rows=n, text_bytes=os.path.getsize(dev_path), reps=args.reps, host_to_csv_ms=host_ms, dev_call_ms=call_ms,
                dev_call_median_ms=float(np.median(call_ms)), host_cpus=len(os.sched_getaffinity(0)),
                host_copy_threads=12, equal=True)
    for k, v in parts.items():
        line[f"dev_{k}_ms"] = v
        line[f"dev_{k}_median_ms"] = float(np.median(v))
    line["ratio"] = host_ms / line["dev_call_median_ms"]
    emit(line)
    os.remove(host_path)
    os.remove(dev_path)
    del frame, cols
if not args.dir:
    os.rmdir(tmp)
