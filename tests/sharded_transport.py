"""Ranks as threads of one process: the in-process transport of tests/test_gpu_sharded.py and tests/test_gpu_sharded_small.py.

`ThreadTransport` stands in for RCCL: every rank is a thread with its own context and stream; a collective waits for every rank's
stream, then adds (all-reduce) or lays out (all-gather) the ranks' device buffers in rank order.  `run_ranks` arms a pool of contexts
with a case's world and rank (`chicdiff_hip_set_allreduce` re-arms a context: no context is opened per case), runs one function per
rank, and disarms them again.  A rank that raises aborts the barrier, so its peers' collectives fail instead of waiting for it; the
threads are joined with a timeout and a rank still alive fails the test."""
import ctypes as C
import threading


class ThreadTransport:
    """In-process stand-in for RCCL: the ranks are threads, each with its own context and stream; a collective waits for
    every rank's stream, then adds (all-reduce) or lays out (all-gather) the ranks' device buffers in rank order."""

    def __init__(self, world, torch, device, timeout=300):
        from chicdiff_amd.dist import ALLGATHER_FN, ALLREDUCE_FN, _RawDevice
        self.world, self.torch = world, torch
        self.barrier = threading.Barrier(world, timeout=timeout)
        self.slots = [None] * world
        self.error = None
        self.reduce_fns, self.gather_fns = [], []
        view = lambda ptr, count: torch.as_tensor(_RawDevice(int(ptr), int(count)), device=device)

        def make(rank):
            def reduce_cb(_u, ptr, count):
                try:
                    self.slots[rank] = view(ptr, count)
                    torch.cuda.synchronize()       # this rank's stream has produced the buffer (device-wide: simplest)
                    self.barrier.wait()
                    if rank == 0:
                        acc = self.slots[0].clone()
                        for r in range(1, world):  # fixed order
                            acc += self.slots[r]
                        self.total = acc
                        torch.cuda.synchronize()
                    self.barrier.wait()
                    self.slots[rank].copy_(self.total)
                    torch.cuda.synchronize()
                    self.barrier.wait()
                    return 0
                except Exception as e:  # noqa: BLE001 — must not cross the C boundary
                    self.error = e
                    return 1

            def gather_cb(_u, send, recv, count):
                try:
                    self.slots[rank] = view(send, count)
                    torch.cuda.synchronize()
                    self.barrier.wait()
                    out = view(recv, int(count) * world)
                    for r in range(world):
                        out[r * int(count):(r + 1) * int(count)].copy_(self.slots[r])
                    torch.cuda.synchronize()
                    self.barrier.wait()
                    return 0
                except Exception as e:  # noqa: BLE001
                    self.error = e
                    return 1

            return ALLREDUCE_FN(reduce_cb), ALLGATHER_FN(gather_cb)

        for r in range(world):
            a, g = make(r)
            self.reduce_fns.append(a)
            self.gather_fns.append(g)


def disarm(c):
    """back to the single-process path (fn = NULL also clears the all-gather hook)"""
    from chicdiff_amd.dist import ALLREDUCE_FN
    c._check(c.lib.chicdiff_hip_set_allreduce(c.h, C.cast(None, ALLREDUCE_FN), None, 1, 0))


def run_ranks(ctxs, world, fn, allgather=True, barrier_timeout=60, join_timeout=120):
    """fn(c, rank) on ctxs[rank], rank = 0 .. world - 1, one thread each, over a ThreadTransport; `allgather=False` registers no
    all-gather hook (the library then gathers by a sum-all-reduce over zero-filled arrays).  Returns the ranks' results in rank order."""
    import torch
    tr = ThreadTransport(world, torch, ctxs[0].device, timeout=barrier_timeout)
    results, errors = [None] * world, [None] * world

    def run(rank):
        try:
            c = ctxs[rank]
            c._check(c.lib.chicdiff_hip_set_allreduce(c.h, tr.reduce_fns[rank], None, world, rank))
            if allgather:
                c._check(c.lib.chicdiff_hip_set_allgather(c.h, tr.gather_fns[rank], None))
            results[rank] = fn(c, rank)
        except Exception as e:  # noqa: BLE001
            errors[rank] = e
            tr.barrier.abort()  # the peers' collectives fail instead of waiting for this rank for ever

    threads = [threading.Thread(target=run, args=(r,), daemon=True) for r in range(world)]
    for t in threads:
        t.start()
    for t in threads:
        t.join(join_timeout)
    assert not any(t.is_alive() for t in threads), "a rank is stuck in a collective"
    for c in ctxs[:world]:
        disarm(c)   # (the transport's callbacks go away with it)
    assert all(e is None for e in errors) and tr.error is None, (errors, tr.error)
    return results
