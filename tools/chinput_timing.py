"""f2, text part: read_chinput(device=False) (host threads parse the text) beside read_chinput(device=True) (the text goes up as
bytes and two kernels parse it) in one process, alternating, on synthetic .chinput files in the reference's five-column format.

    python3 tools/chinput_timing.py [--rows 4000000,40000000] [--reps 5] [--dir DIR] [--out profiles/r21_chinput_timing.jsonl]

Files: '#' comment line, header `baitID otherEndID N otherEndLen distSign`, tab-separated rows, 10 % of distSign NA, baits ascending
within a block.  A file of more than 4 M rows repeats one block of 4 M rows (written once, appended many times): the parsers' work per
row does not depend on it.  Each file is read once untimed (page cache warm, buffers of the context grown), then ``reps`` times by
each path, alternating.  No bait filter (every row reaches the key table), so both paths sort the same rows.

One JSON line per file:
  file_bytes, rows, host_threads (the context's host_copy_threads: parser threads of the host path, copy threads of the upload)
  host_call_ms      whole read_chinput(device=False) calls, host clock: parse, upload of the three columns, key table
  dev_call_ms       whole read_chinput(device=True) calls: header, upload of the text, mark, scan, parse, key table
  dev_split_ms      a second round of device reads with the library's event timer on: chinput_upload (first copy into the staging
                    area to the last DMA's end, on the stream), chinput_mark, chinput_scan, chinput_parse, and count_table behind them
  equal             the two paths' key tables are equal (asserted)"""
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
ap.add_argument("--rows", default="4000000,40000000")
ap.add_argument("--reps", type=int, default=5)
ap.add_argument("--dir", default=None)
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r21_chinput_timing.jsonl"))
args = ap.parse_args()

BLOCK = 4_000_000


def block_text(n, seed=21):
    import pandas as pd
    rng = np.random.default_rng(seed)
    bait = np.sort(rng.integers(1, 800_000, n))
    dist = rng.integers(-10 ** 6, 10 ** 6, n).astype(object)
    dist[rng.random(n) < 0.1] = "NA"
    x = pd.DataFrame({"baitID": bait, "otherEndID": rng.integers(1, 840_000, n), "N": rng.geometric(0.3, n),
                      "otherEndLen": rng.integers(100, 20000, n), "distSign": dist})
    return x.to_csv(sep="\t", index=False, header=False).encode()


def write_file(path, n):
    block = block_text(min(n, BLOCK))
    with open(path, "wb") as f:
        f.write(b"#\tsamplename=x\tbamname=x.bam\tbaitmapfile=b.baitmap\tdigestfile=d.rmap\n")
        f.write(b"baitID\totherEndID\tN\totherEndLen\tdistSign\n")
        for _ in range(max(1, n // BLOCK)):
            f.write(block)
    return os.path.getsize(path)


import torch  # noqa: E402

from chicdiff_amd import hip  # noqa: E402

ctx = hip.HipContext(0)
host_threads = 12                         # the context's default host_copy_threads (include/chicdiff_hip.h)
tmp = tempfile.mkdtemp(dir=args.dir)
for n in (int(r) for r in args.rows.split(",")):
    path = os.path.join(tmp, f"synthetic_{n}.chinput")
    t0 = time.perf_counter()
    nbytes = write_file(path, n)
    print(f"# {path}: {nbytes} bytes written in {time.perf_counter() - t0:.1f} s", file=sys.stderr, flush=True)
    line = dict(rows=max(1, n // BLOCK) * min(n, BLOCK), file_bytes=nbytes, host_threads=host_threads, reps=args.reps,
                host_cpus=len(os.sched_getaffinity(0)))

    def timed(device):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        keys, vals, nrows = ctx.read_chinput(path, None, device=device)
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3, keys, vals, nrows

    _, hk, hv, hn = timed(False)          # untimed: page cache, staging areas, device buffers
    _, dk, dv, dn = timed(True)
    assert hn == dn == line["rows"] and torch.equal(hk, dk) and torch.equal(hv, dv)
    line["equal"] = True
    del hk, hv, dk, dv
    host_ms, dev_ms = [], []
    for _ in range(args.reps):
        host_ms.append(timed(False)[0])
        dev_ms.append(timed(True)[0])
    line.update(host_call_ms=host_ms, host_call_median_ms=float(np.median(host_ms)), dev_call_ms=dev_ms,
                dev_call_median_ms=float(np.median(dev_ms)))
    ctx.enable_timing(True)
    split = {}
    for _ in range(args.reps):
        import ctypes as C
        nrows = C.c_int64(0)
        ctx._check(ctx.lib.chicdiff_hip_chinput_read_dev(ctx.h, os.fsencode(path), C.byref(nrows)))
        for k, (ms, _) in ctx.kernel_times().items():
            split.setdefault(k, []).append(ms)
        keys = torch.empty(nrows.value, dtype=torch.int64, device=ctx.device)
        vals = torch.empty(nrows.value, dtype=torch.int32, device=ctx.device)
        nk = C.c_int64(0)
        ctx._check(ctx.lib.chicdiff_hip_chinput_table_dev(ctx.h, None, 0, keys.data_ptr(), vals.data_ptr(), C.byref(nk)))
        for k, (ms, _) in ctx.kernel_times().items():
            split.setdefault(k, []).append(ms)
        del keys, vals
    ctx.enable_timing(False)
    line["dev_split_ms"] = split
    line["dev_split_median_ms"] = {k: float(np.median(v)) for k, v in split.items()}
    print(json.dumps(line), flush=True)
    with open(args.out, "a") as f:
        f.write(json.dumps(line) + "\n")
    os.remove(path)
os.rmdir(tmp)
ctx.close()
