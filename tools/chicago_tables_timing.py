"""The Chicago background tables: the host twin (pipeline.background_tables, pandas) beside the device path
(pipeline.background_tables_dev -> chicdiff_hip_chicago_tables_dev) at the size of real Chicago tables.

    python3 tools/chicago_tables_timing.py [--rows 2000000,20000000] [--S 4] [--reps 7] [--out FILE] [--no-host]

Geometry: a human-sized restriction map (840 000 fragments, id_min = 1), 22 000 baits, every row an other end within 3 000 fragments
of its bait; 8 x 8 (tblb, tlb) label bins, 75 distance bins, refBinMean a function of distbin; 10 % of the tlb labels NA.  The label
columns are pandas categoricals (the cheapest form for both sides).  ONE table is generated per size and serves as every one of the
S replicates — the work of either side does not depend on the replicates being different.  Each size runs keyed by (baitID,
otherEndID), as Chicago writes its tables, and shuffled.

One JSON line per size and row order:
  host_twin_ms      one run of pipeline.background_tables on this host's CPU (S replicates)
  dev_call_ms       ``reps`` runs of pipeline.background_tables_dev: label codes, upload of the nine columns, kernels, the status
                    read-back, the cubic fit of the distance function — host clock around a call that ends synchronised
  codes_ms          the share of that spent in pipeline.chicago_codes (host)
  kernels_ms        ``reps`` runs of the S calls of HipContext.chicago_tables on columns already on the device: the library's own
                    event timers, summed over the replicates; init / pass1 / pass2 (pass 2 with the epilogue) apart
  *_no_merge        the same with the wave-level run merge switched off (option "chicago_tables_run_merge" = 0)
  pass1_bytes / pass2_bytes   the streamed bytes of the algorithm, 28 and 16 per row and replicate (the slots, 16 nid bytes, and the
                    winners' gathers are not counted), and pass*_TBps = those bytes over the median pass time"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

ap = argparse.ArgumentParser()
ap.add_argument("--rows", default="2000000,20000000")
ap.add_argument("--S", type=int, default=4)
ap.add_argument("--reps", type=int, default=7)
ap.add_argument("--out", default=None)
ap.add_argument("--no-host", action="store_true")
args = ap.parse_args()

NID, ID_MIN, NBAITS, NLEV, NBIN = 840000, 1, 22000, 8, 75


def emit(line):
    print(json.dumps(line), flush=True)
    if args.out:
        with open(args.out, "a") as f:
            f.write(json.dumps(line) + "\n")


def make(n, seed=16):
    import pandas as pd
    rng = np.random.default_rng(seed)
    baits = np.sort(rng.choice(np.arange(ID_MIN + 3000, ID_MIN + NID - 3000), NBAITS, replace=False))
    b = baits[rng.integers(0, NBAITS, n)]
    o = b + rng.integers(1, 3001, n) * rng.choice([-1, 1], n)
    order = np.lexsort((o, b))
    b, o = b[order].astype(np.int32), o[order].astype(np.int32)
    levB, levL = [f"tb{k}" for k in range(NLEV)], [f"tl{k}" for k in range(NLEV)]
    tb_of, tl_of = rng.integers(0, NLEV, NID + 1), np.where(rng.random(NID + 1) < 0.1, -1, rng.integers(0, NLEV, NID + 1))
    T = np.exp(rng.normal(-2.5, 0.4, (NLEV, NLEV)))
    tb, tl = tb_of[b], tl_of[o]
    k = np.minimum(np.abs(o - b) // 40, NBIN - 1)
    refmean = np.exp(3.0 - 0.9 * np.log(np.arange(1, NBIN + 1)))
    return pd.DataFrame({"baitID": b, "otherEndID": o, "s_j": np.exp(rng.normal(0, 0.25, NID + 1))[b], "s_i": np.exp(rng.normal(0, 0.25, NID + 1))[o],
                         "tblb": pd.Categorical.from_codes(tb, levB), "tlb": pd.Categorical.from_codes(tl, levL),
                         "Tmean": np.where(tl >= 0, T[tb, np.maximum(tl, 0)], np.nan),
                         "distbin": pd.Categorical.from_codes(k, [f"bin{j:03d}" for j in range(NBIN)]), "refBinMean": refmean[k]})


import torch  # noqa: E402

from chicdiff_amd import hip, pipeline  # noqa: E402

ctx = hip.HipContext(0)
ctx.enable_timing(True)
dev = lambda a, t: torch.from_numpy(np.ascontiguousarray(a, dtype=t)).to(ctx.device)
S = args.S
for n in (int(r) for r in args.rows.split(",")):
    keyed = make(n)
    for order in ("keyed", "shuffled"):
        x = keyed if order == "keyed" else keyed.sample(frac=1.0, random_state=1).reset_index(drop=True)
        xs = [x] * S
        line = dict(rows=n, S=S, order=order, nid=NID, label_bins=[NLEV, NLEV], distance_bins=NBIN, reps=args.reps)
        print(f"# {n} rows, {order}: device", file=sys.stderr, flush=True)
        codes_ms = []
        real_codes = pipeline.chicago_codes

        def timed_codes(xs_):
            t0 = time.perf_counter()
            r = real_codes(xs_)
            codes_ms.append((time.perf_counter() - t0) * 1e3)
            return r

        pipeline.chicago_codes = timed_codes
        call_ms = []
        for rep in range(args.reps + 2):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            got = pipeline.background_tables_dev(xs, ID_MIN, NID, ctx)
            torch.cuda.synchronize()
            call_ms.append((time.perf_counter() - t0) * 1e3)
        pipeline.chicago_codes = real_codes
        line.update(dev_call_ms=call_ms[2:], dev_call_median_ms=float(np.median(call_ms[2:])), codes_ms=codes_ms[2:],
                    codes_median_ms=float(np.median(codes_ms[2:])))
        # kernels alone: one replicate's columns on the device, S calls per repeat
        cd = pipeline.chicago_codes([x])
        cols = [dev(x["baitID"].to_numpy(), np.int32), dev(x["otherEndID"].to_numpy(), np.int32)]
        cols += [dev(x[c].to_numpy(np.float64), np.float64) for c in ("s_j", "s_i", "Tmean", "refBinMean")]
        cols += [dev(cd[c][0], np.int32) for c in ("tblb", "tlb", "distbin")]
        sj, si = (torch.empty((S, NID), dtype=torch.float64, device=ctx.device) for _ in range(2))
        tbo, tlo = (torch.empty((S, NID), dtype=torch.int32, device=ctx.device) for _ in range(2))
        T = torch.empty((S, NLEV, NLEV), dtype=torch.float64, device=ctx.device)
        for merge, tag in ((1, ""), (0, "_no_merge")):
            ctx.set_option("chicago_tables_run_merge", merge)
            per = {"init": [], "pass1": [], "pass2": []}
            for rep in range(args.reps + 2):
                tot = dict.fromkeys(per, 0.0)
                for s in range(S):
                    _, flag = ctx.chicago_tables(*cols, ID_MIN, cd["ndistbin"][0], sj[s], si[s], tbo[s], tlo[s], T[s])
                    assert not flag
                    for k in tot:
                        tot[k] += ctx.last_chicago_tables_ms[k]
                if rep >= 2:
                    for k in per:
                        per[k].append(tot[k])
            total = [a + b + c for a, b, c in zip(per["init"], per["pass1"], per["pass2"])]
            line["kernels_ms" + tag] = total
            line["kernels_median_ms" + tag] = float(np.median(total))
            for k in per:
                line[f"{k}_median_ms" + tag] = float(np.median(per[k]))
            line["pass1_TBps" + tag] = 28.0 * n * S / (np.median(per["pass1"]) * 1e-3) / 1e12
            line["pass2_TBps" + tag] = 16.0 * n * S / (np.median(per["pass2"]) * 1e-3) / 1e12
        ctx.set_option("chicago_tables_run_merge", 1)
        line.update(pass1_bytes=28 * n * S, pass2_bytes=16 * n * S)
        for k, a in (("sj", sj), ("si", si), ("tblb", tbo), ("tlb", tlo), ("T", T)):     # the kernels-only run computed the call's tables
            assert torch.equal(a.view(torch.int64) if a.dtype == torch.float64 else a, got[k].view(torch.int64) if a.dtype == torch.float64 else got[k]), k
        del cols
        if not args.no_host:
            print(f"# {n} rows, {order}: host twin", file=sys.stderr, flush=True)
            t0 = time.perf_counter()
            want = pipeline.background_tables(xs[:1], ID_MIN, NID)
            one = (time.perf_counter() - t0) * 1e3
            print(f"# one replicate: {one:.0f} ms", file=sys.stderr, flush=True)
            t0 = time.perf_counter()
            for s in range(1, S):
                pipeline.background_tables(xs[s:s + 1], ID_MIN, NID)
                print(f"# replicate {s + 1} done", file=sys.stderr, flush=True)
            line["host_twin_ms"] = one + (time.perf_counter() - t0) * 1e3
            line["host_cpus"] = len(os.sched_getaffinity(0))
            for k in ("sj", "si", "T"):                                                # ... and the device's are the twin's
                assert np.array_equal(np.nan_to_num(want[k][0], nan=-1.0).view(np.int64), np.nan_to_num(got[k][0].cpu().numpy(), nan=-1.0).view(np.int64)), k
            assert np.array_equal(want["tblb"][0], got["tblb"][0].cpu().numpy()) and np.array_equal(want["tlb"][0], got["tlb"][0].cpu().numpy())
            assert np.array_equal(want["distfun"][0].view(np.int64), got["distfun"][0].view(np.int64))
        emit(line)
        del got, x, xs
