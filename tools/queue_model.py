"""CPU model of the gene-wise line search's row queue: which visit order ends the launch soonest (no GPU needed).

The oracle's dispGeneIter is the number of evaluations a row's search takes, dispInit its start value; with the group means
that gives every row's schedule score (alpha_init * smaller group mean) and its cost.  The model: W waves x 64 lanes, one
evaluation per lane and tick, all lanes in step; a free lane takes the wave's next dealt-out row (the static deal "A": the
classes below score 0.316, in groups of eight entries round-robin over the waves), then the next row of the queue.  Time =
ticks while the queue has rows x the bulk tick + ticks after x the drain tick.  It is crude (synchronous ticks, one price per
drain tick: it put the three-waves launch of the six-class order at 1.22 ms where 1.43 was measured) — use it to compare
ORDERS for a shape (other S, other class edges), not to predict a time.

usage: python tools/queue_model.py [--rows 200000] [--samples 8] [--tile-to 2000000] [--waves-per-simd 2] [--edges e1,e2,...]
                                   [--fillers FRONT ALONE FILLER [--filler-stop 100 85 ...]]
  --fillers: also the two-ended queue of the front-waves-and-fillers launch (two front waves + one filler per SIMD), with a tick
             length per role in us, for the stop shares given — the order of the settings before GPU time is spent on them
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


def simulate_two_ended(cost, order, n_deal, n_back, fronts, fillers, pace_front, pace_front_alone, pace_fill, tick_drain, stop_share):
    """Front waves and fillers (disp_kernels.hip): `fronts` waves take the static deal and the queue from its head and tick every
    pace_front us while any filler is at work (pace_front_alone after that, tick_drain once the queue is empty); `fillers` waves tick
    every pace_fill us and take rows from the queue's END, down to schedule position n_back (the first row that cannot be long), while
    the head has not passed stop_share of the front's own rows.  Rows, not chunks; each group ticks in step.  Returns the time the
    queue ran empty, the time the last front wave / the last filler finished (us) and the share of the evaluations the fillers did."""
    L = 64
    queue = cost[order[n_deal:]].astype(np.int32)
    kb = max(n_back - n_deal, 0)
    stop_head = len(queue) + 1 if stop_share >= 100 else int(np.ceil(min(kb, len(queue)) * stop_share / 100.0))
    dealt = cost[order[:n_deal]].astype(np.int32)
    g = np.arange(len(dealt)) // DEAL_GROUP
    deal_of = [dealt[g % fronts == w] for w in range(fronts)] if n_deal else [np.zeros(0, np.int32)] * fronts
    deal_len = np.array([len(x) for x in deal_of])
    deal = np.zeros((fronts, max(int(deal_len.max()), 1)), np.int32)
    for w, x in enumerate(deal_of):
        deal[w, :len(x)] = x
    deal_pos = np.zeros(fronts, np.int64)
    rem_f, rem_b = np.zeros((fronts, L), np.int32), np.zeros((max(fillers, 1), L), np.int32)
    head, tail = 0, len(queue)
    t_f = t_b = 0.0
    t_empty = None
    end_f = end_b = 0.0
    ev_f = ev_b = 0
    fill_on = fillers > 0 and stop_head > 0 and kb < len(queue)
    while True:
        if fill_on and t_b <= t_f:  # the fillers' tick
            free = rem_b == 0
            can = max(tail - max(head, kb), 0) if head < stop_head else 0
            take = min(int(free.sum()), can)
            if take:
                idx = np.flatnonzero(free.ravel())[:take]
                rem_b.ravel()[idx] = queue[tail - take:tail][::-1]
                tail -= take
            busy = rem_b > 0
            if not busy.any():
                fill_on = False
                continue
            ev_b += int(busy.sum())
            rem_b -= busy
            t_b += pace_fill
            end_b = t_b
            continue
        free = rem_f == 0
        nfree = free.sum(1)
        from_deal = np.minimum(nfree, deal_len - deal_pos)
        rank = np.cumsum(free, 1) - 1
        take_deal = free & (rank < from_deal[:, None])
        rem_f = np.where(take_deal, np.take_along_axis(deal, np.minimum(deal_pos[:, None] + rank, deal.shape[1] - 1), 1), rem_f)
        deal_pos += from_deal
        need = nfree - from_deal
        start = head + np.cumsum(need) - need
        qi = start[:, None] + rank - from_deal[:, None]
        take_q = free & ~take_deal & (qi < tail)
        if len(queue):
            rem_f = np.where(take_q, queue[np.minimum(qi, len(queue) - 1)], rem_f)
        head = min(head + int(need.sum()), tail)
        if t_empty is None and head >= tail and np.all(deal_pos >= deal_len):
            t_empty = t_f
        busy = rem_f > 0
        if not busy.any():
            if not fill_on:
                break
            t_f = t_b + 1e-9  # (front waves are done: only the fillers' ticks are left)
            continue
        ev_f += int(busy.sum())
        rem_f -= busy
        t_f += tick_drain if t_empty is not None else (pace_front if fill_on else pace_front_alone)
        end_f = t_f
    return t_empty, end_f, end_b, ev_b / max(ev_f + ev_b, 1)


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--rows", type=int, default=200000, help="rows the oracle fits")
    ap.add_argument("--samples", type=int, default=8)
    ap.add_argument("--tile-to", type=int, default=2000000, help="rows of the modelled launch (the fitted rows, repeated and shuffled)")
    ap.add_argument("--waves-per-simd", type=int, default=2)
    ap.add_argument("--tick-us", type=float, nargs=2, default=None, help="bulk and drain tick (default 8.0 / 10.56 for two / three waves, 4.4)")
    ap.add_argument("--edges", type=str, default=None)
    ap.add_argument("--fillers", type=float, nargs=3, default=None, metavar=("FRONT", "ALONE", "FILLER"),
                    help="also model two front waves + one filler per SIMD on the default order: us per tick of a front wave beside a filler, of a front "
                         "wave once the fillers are gone, and of a filler (measured at 2 M x 8: 8.6 7.97 18.8)")
    ap.add_argument("--filler-stop", type=int, nargs="*", default=[100, 85, 70, 40], help="stop shares (percent) to model with --fillers")
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
    if a.fillers:
        cls = orders["1/8 decade, minDisp starts before 3.16"]
        order = np.argsort(cls, kind="stable")
        n_deal = int(((score < DEAL_BELOW) & ~at_min).sum())
        n_back = int((at_min | (score < 3.16)).sum())  # schedule position of the first row of score >= 3.16
        pf, pa, pb = a.fillers
        print(f"front waves and fillers (2 + 1 per SIMD), ticks {pf} / {pa} / {pb} us, drain {drain} us; rows fillers may take: {len(cost) - n_back}:")
        for share in [0] + list(a.filler_stop):
            te, ef, eb, part = simulate_two_ended(cost, order, n_deal, n_back, 256 * 8, 256 * 4, pf, pa, pb, drain, share)
            print(f"  stop share {share:3d}: queue empty at {te / 1e3:.3f} ms, last front wave out {ef / 1e3:.3f}, last filler out {eb / 1e3:.3f}, fillers did {part * 100:.1f} % of the evaluations")


if __name__ == "__main__":
    main()
