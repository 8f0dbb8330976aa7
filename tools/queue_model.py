"""CPU model of the gene-wise line search's row queue: which visit order ends the launch soonest (no GPU needed).

The oracle's dispGeneIter is the number of evaluations a row's search takes, dispInit its start value; with the group means
that gives every row's schedule score (alpha_init * smaller group mean) and its cost.  The model: W waves x 64 lanes, one
evaluation per lane and tick, all lanes in step; a free lane takes the wave's next dealt-out row (the static deal "A": the
classes below score 0.316, in groups of eight entries round-robin over the waves), then the next row of the queue.  Time =
ticks while the queue has rows x the bulk tick + ticks after x the drain tick.  It is crude (synchronous ticks, one price per
drain tick: it put the three-waves launch of the six-class order at 1.22 ms where 1.43 was measured) — use it to compare
ORDERS for a shape (other S, other class edges), not to predict a time.

usage: python tools/queue_model.py [--rows 200000] [--samples 8] [--tile-to 2000000] [--waves-per-simd 2] [--edges e1,e2,...]
  --edges: score edges of an order to try besides the built-in ones (rows at minDisp and scores above the last edge go last)"""
import argparse
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
SIX = [0.1, 0.316, 1.0, 3.16, 10.0]
FINE = [0.0316, 0.0422, 0.0562, 0.0750, 0.1, 0.1334, 0.1778, 0.2371, 0.316, 0.4217, 0.5623, 0.7499, 1.0, 1.3335, 1.7783, 2.3714,
        3.16, 4.2170, 5.6234, 7.4989, 10.0]  # chicdiff_amd/csrc/common.h: sched_class
DEAL_BELOW, DEAL_GROUP = 0.316, 8


def classes(score, at_min, edges, min_before=None):
    """class per row: edges not above the score; minDisp starts last, or (min_before = a score) in front of the rows from that score on"""
    edges = np.asarray(edges)
    c = 2 * np.searchsorted(edges, score, side="right")  # even numbers: room for the minDisp starts in between
    last = 2 * len(edges)
    return np.where(at_min, last if min_before is None else 2 * np.searchsorted(edges, min_before, side="right") - 1, c)


def simulate(cost, order, n_deal, waves, tick_bulk, tick_drain):
    """cost[row] evaluations; order = rows in visit order, the first n_deal of them dealt out statically"""
    L = 64
    groups = (n_deal + DEAL_GROUP - 1) // DEAL_GROUP
    per_wave = (groups + waves - 1) // waves * DEAL_GROUP
    deal = np.zeros((waves, max(per_wave, 1)), dtype=np.int32)
    deal_len = np.zeros(waves, dtype=np.int64)
    g = np.arange(groups)
    for k in range(DEAL_GROUP):  # entry k of group g belongs to wave g mod W, slot (g div W) * 8 + k
        pos = g * DEAL_GROUP + k
        ok = pos < n_deal
        deal[g[ok] % waves, (g[ok] // waves) * DEAL_GROUP + k] = cost[order[pos[ok]]]
    np.add.at(deal_len, g % waves, np.minimum(DEAL_GROUP, n_deal - g * DEAL_GROUP))
    # (a wave's dealt entries are contiguous from slot 0 except in its last group, which only the last wave can hold short)
    queue = cost[order[n_deal:]].astype(np.int32)
    rem = np.zeros((waves, L), dtype=np.int32)
    deal_pos = np.zeros(waves, dtype=np.int64)
    head, tick, tick_empty, evals = 0, 0, None, 0
    while True:
        free = rem == 0
        nfree = free.sum(1)
        from_deal = np.minimum(nfree, deal_len - deal_pos)
        need = nfree - from_deal
        start = head + np.cumsum(need) - need
        rank = np.cumsum(free, 1) - 1
        take_deal = free & (rank < from_deal[:, None])
        idx = np.minimum(deal_pos[:, None] + rank, deal.shape[1] - 1)
        rem = np.where(take_deal, np.take_along_axis(deal, idx, 1), rem)
        qi = start[:, None] + rank - from_deal[:, None]
        take_q = free & ~take_deal & (qi < len(queue))
        rem = np.where(take_q, queue[np.minimum(qi, max(len(queue) - 1, 0))] if len(queue) else 0, rem)
        deal_pos += from_deal
        head = min(head + int(need.sum()), len(queue))
        if tick_empty is None and head >= len(queue) and np.all(deal_pos >= deal_len):
            tick_empty = tick
        busy = rem > 0
        if not busy.any():
            break
        evals += int(busy.sum())
        rem = rem - busy
        tick += 1
    return tick_empty, tick, (tick_empty * tick_bulk + (tick - tick_empty) * tick_drain) / 1e3, evals


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--rows", type=int, default=200000, help="rows the oracle fits")
    ap.add_argument("--samples", type=int, default=8)
    ap.add_argument("--tile-to", type=int, default=2000000, help="rows of the modelled launch (the fitted rows, repeated and shuffled)")
    ap.add_argument("--waves-per-simd", type=int, default=2)
    ap.add_argument("--tick-us", type=float, nargs=2, default=None, help="bulk and drain tick (default 8.0 / 10.56 for two / three waves, 4.4)")
    ap.add_argument("--edges", type=str, default=None)
    a = ap.parse_args()
    from chicdiff_amd import synth
    from oracle import oracle

    d = synth.make(a.rows, a.samples)
    ref = oracle.nbglm_fit(d["counts"], d["nf"], d["group"])
    g = np.asarray(d["group"])
    q = d["counts"] / d["nf"]
    gmin = np.minimum(q[:, g == 0].mean(1), q[:, g == 1].mean(1)) if g.any() else q.mean(1)
    live = ref["allZero"] == 0
    a0, cost, gmin = ref["dispInit"][live], np.maximum(ref["dispGeneIter"][live], 1), gmin[live]
    min_disp = 1e-8
    at_min = ~(a0 > 1.5 * min_disp)
    score = a0 * gmin
    print(f"{a.rows} x {a.samples}: {live.sum()} rows searched, {cost.sum()} evaluations, {np.mean(cost >= 50) * 100:.2f} % of the rows take >= 50 "
          f"({cost[cost >= 50].sum() / cost.sum() * 100:.1f} % of the evaluations), {at_min.mean() * 100:.1f} % start at minDisp")
    print("evaluations per class of the six-class order (p50 / p90 / p99 / max, share of rows, share taking >= 50):")
    six = classes(score, at_min, SIX) // 2
    for c in range(6):
        m = (six == c) & ~at_min
        if m.any():
            print(f"  class {c}: {m.mean() * 100:5.1f} % of rows, " + " / ".join("%d" % v for v in np.percentile(cost[m], [50, 90, 99, 100])) + f", long {np.mean(cost[m] >= 50) * 100:.3f} %")
    print(f"  minDisp starts: {at_min.mean() * 100:5.1f} % of rows, " + " / ".join("%d" % v for v in np.percentile(cost[at_min], [50, 90, 99, 100])))
    reps = max(1, a.tile_to // len(cost))
    perm = np.random.default_rng(1).permutation(len(cost) * reps)
    cost, score, at_min = np.tile(cost, reps)[perm], np.tile(score, reps)[perm], np.tile(at_min, reps)[perm]
    waves = 256 * 4 * a.waves_per_simd
    bulk, drain = a.tick_us if a.tick_us else ((8.0 if a.waves_per_simd <= 2 else 10.56), 4.4)
    orders = {"natural order": np.zeros(len(cost), dtype=np.int64), "six half-decade classes": classes(score, at_min, SIX),
              "1/8-decade classes": classes(score, at_min, FINE), "1/8 decade, minDisp starts before 3.16": classes(score, at_min, FINE, 3.16),
              "rows with >= 50 evaluations first (oracle)": np.where(cost >= 50, 0, 2 + classes(score, at_min, SIX))}
    if a.edges:
        orders["--edges"] = classes(score, at_min, [float(x) for x in a.edges.split(",")])
    print(f"model of {len(cost)} rows on {waves} waves ({a.waves_per_simd} per SIMD), tick {bulk} / {drain} us:")
    for name, cls in orders.items():
        order = np.argsort(cls, kind="stable")
        n_deal = 0 if name == "natural order" else int(((score < DEAL_BELOW) & ~at_min).sum())
        if name.startswith("rows with"):
            n_deal = int(((cost >= 50) | ((score < DEAL_BELOW) & ~at_min)).sum())
        te, t, ms, evals = simulate(cost, order, n_deal, waves, bulk, drain)
        print(f"  {name:45s} queue empty at tick {te:4d}, end {t:4d}  (~{ms:.2f} ms), {evals} evaluations")


if __name__ == "__main__":
    main()
