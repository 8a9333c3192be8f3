"""Rank functions of the two-phase all-reduce tests (``tests/parallel/test_twophase.py``), run by
``testing.distributed.run_ranks`` on ranks that share ``cuda:0`` (gloo bootstrap,
``IMITATION_AMD_ONESHOT=1``). Module-level so the spawn start method can pickle them."""

from __future__ import annotations

import numpy as np
import torch as th

from imitation_amd.testing import dist_workers
from imitation_amd.utils import graphs


def _small_comm(slot_bytes, self_test=False):
    """A two-phase communicator with a deliberately small slot next to the process-wide one-shot
    communicator (collective): block and shard edges are then reached with small arrays."""
    from imitation_amd.parallel import oneshot

    base = oneshot.get()
    assert base is not None, "one-shot path not set up"
    c = oneshot.TwoPhaseComm(base._C, base.rank, base.world, base.device, slot_bytes, base.timeout_s)
    if self_test:
        c = oneshot.adopt(c, "1")  # raises with the reason when the start-up self-test fails
    return base, c


def _close(c):
    from imitation_amd.parallel import dist as pdist

    th.cuda.synchronize(c.device)
    pdist.barrier()  # no peer still has a kernel reading this rank's region
    c.close()


def _data(seed, rank, n, extra=0, f64=False):
    x = np.random.default_rng(seed * 100 + rank * 7 + n + extra).normal(size=n)
    return x if f64 else x.astype(np.float32)


def twophase_worker(rank, world, slot_bytes, sizes, f64_sizes, scale, seed):
    """Rank-seeded normal buckets of ``sizes`` (fp32) and ``f64_sizes`` (fp64, interleaved with fp32
    calls) through the two-phase kernel, then one captured full-slot call replayed three times
    with fresh inputs. Returns this rank's results for the parent to compare bitwise."""
    _, c = _small_comm(slot_bytes, self_test=True)
    dev = c.device
    out = {"eager": [], "f64": [], "graph": [], "blocks": [c.blocks(n) for n in sizes]}
    for n in sizes:
        x = th.as_tensor(_data(seed, rank, n), device=dev)
        c.allreduce_(x, scale)
        out["eager"].append(x.cpu().numpy())
    for n in f64_sizes:
        x = th.as_tensor(_data(seed, rank, n, 5, f64=True), device=dev)
        c.allreduce_(x, scale)
        y = th.ones(n + 3, device=dev)
        c.allreduce_(y)
        out["f64"].append(x.cpu().numpy())
    buf = th.zeros(slot_bytes // 4, device=dev)
    side = th.cuda.Stream(device=dev)
    side.wait_stream(th.cuda.current_stream(dev))
    g = th.cuda.CUDAGraph()
    with th.cuda.stream(side):
        with graphs.capture(g, stream=side):
            c.allreduce_(buf, scale)
    th.cuda.current_stream(dev).wait_stream(side)
    for rep in range(3):
        buf.copy_(th.as_tensor(_data(seed, rank, buf.numel(), 1000 + rep)))
        g.replay()
        out["graph"].append(buf.cpu().numpy())
    th.cuda.synchronize(dev)
    out["error"] = c.error()
    del g
    _close(c)
    return out


def twophase_stress_worker(rank, world, slot_bytes, sizes, iters, seed):
    """Uneven arrival: a random amount of GPU work (and host sleep) on every rank before each of
    ``iters`` reductions, each on the one-shot or the two-phase communicator and of a size of
    ``sizes``, chosen at random (the same choice on every rank). Small integers plus halves: every
    summation order is exact, and every word of every reduction is checked."""
    import time

    one, two = _small_comm(slot_bytes)
    dev = two.device
    rng = np.random.default_rng(seed)  # same sequence on every rank
    local = np.random.default_rng(seed * 31 + rank)  # rank-local load pattern
    a = th.randn(512, 512, device=dev)
    halves = sum(r % 2 for r in range(world)) * 0.5
    bad = th.zeros((), dtype=th.int64, device=dev)
    picks = [0, 0]
    for it in range(iters):
        which = int(rng.integers(0, 2))
        n = int(sizes[int(rng.integers(0, len(sizes)))])
        picks[which] += 1
        for _ in range(int(local.integers(0, 6))):
            a = th.tanh(a @ a * 1e-3)
        if local.random() < 0.2:
            time.sleep(float(local.random()) * 2e-3)
        base = th.arange(n, device=dev, dtype=th.float32) % 97
        x = base * float(rank + 1) + float(it) + 0.5 * (rank % 2)
        (two if which else one).allreduce_(x)
        exp = base * float(world * (world + 1) / 2) + float(it * world) + halves
        bad += (x != exp).sum()
    th.cuda.synchronize(dev)
    res = {"bad_words": int(bad.item()), "error_oneshot": one.error(), "error_twophase": two.error(),
           "picks": picks}
    _close(two)
    return res


def twophase_block_change_worker(rank, world, slot_bytes, reps, seed):
    """Back-to-back two-phase reductions of 1, 3, 128 and 1 blocks in ONE HIP graph, replayed with
    rank-skewed GPU load in front of each replay; every word of every bucket is checked against
    the rank-order sum (one staging and one result area: a block's slice must not depend on the
    call's size, and the two waits must order consecutive calls)."""
    _, c = _small_comm(slot_bytes)
    dev = c.device
    per = c.block_floats()
    sizes = [per // 2 + 3, 2 * per + 5, slot_bytes // 4, 7]
    blocks = [c.blocks(n) for n in sizes]
    bufs = [th.zeros(n, device=dev) for n in sizes]
    side = th.cuda.Stream(device=dev)
    side.wait_stream(th.cuda.current_stream(dev))
    g = th.cuda.CUDAGraph()
    with th.cuda.stream(side):
        with graphs.capture(g, stream=side):
            for b in bufs:
                c.allreduce_(b)
    th.cuda.current_stream(dev).wait_stream(side)
    local = np.random.default_rng(seed * 13 + rank)
    a = th.randn(256, 256, device=dev)
    bad = 0
    for rep in range(reps):
        for i, b in enumerate(bufs):
            b.copy_(th.arange(b.numel(), device=dev, dtype=th.float32) % 89 * float(rank + 1) + float(rep + i))
        for _ in range(int(local.integers(0, 4)) + 3 * ((rep + rank) % 2)):
            a = th.tanh(a @ a * 1e-3)
        g.replay()
        for i, b in enumerate(bufs):
            exp = th.arange(b.numel(), device=dev, dtype=th.float32) % 89 * float(world * (world + 1) / 2) + float((rep + i) * world)
            bad += int((b != exp).sum().item())
    th.cuda.synchronize(dev)
    res = {"bad_words": bad, "blocks": blocks, "error": c.error()}
    del g
    _close(c)
    return res


def twophase_timeout_worker(rank, world, slot_bytes, timeout_s):
    """Rank 0 reduces while rank 1 never joins: the bounded wait must give up, write NaN over the
    whole output and raise the error word; the kernel ends by itself."""
    _, c = _small_comm(slot_bytes)
    res = {}
    if rank == 0:
        c.timeout_s = timeout_s
        x = th.ones(2 * c.block_floats() + 7, device=c.device)
        c.allreduce_(x)
        th.cuda.synchronize(c.device)
        res = {"all_nan": bool(th.isnan(x).all().item()), "error": c.error()}
        try:
            c.check("test", blocking=True)
            res["raised"] = False
        except RuntimeError:
            res["raised"] = True
        res["error_after"] = c.error()
    _close(c)
    return res


def bc_dp_epoch_calls_worker(rank, world, mode):
    """``dist_workers.bc_dp_epoch_worker`` (one short epoch) plus the number of reductions each
    communicator ran for it."""
    from imitation_amd.parallel import oneshot

    out = dist_workers.bc_dp_epoch_worker(rank, world, mode, n_epochs=1, n_rows=32 * 3 + 5)
    out["oneshot_calls"] = oneshot._COMM.calls if oneshot._COMM is not None else 0
    out["twophase_calls"] = oneshot._LARGE.calls if oneshot._LARGE is not None else 0
    out["twophase_error"] = oneshot._LARGE.error() if oneshot._LARGE is not None else 0
    return out


def twophase_timing_worker(rank, world, n_floats, iters, warmup):
    """Informational: median us per reduction of an ``n_floats`` range through the two-phase
    communicator (one launch) against the same range in one-shot chunks of the staging slot,
    measured with device events in the same worker. On one card no link is crossed."""
    from imitation_amd.parallel import dist as pdist
    from imitation_amd.parallel import oneshot

    one = oneshot.get()
    two = oneshot.get_large(n_floats * 4)
    assert one is not None and two is not None
    dev = one.device
    x = th.ones(n_floats, device=dev)
    step = one.stage_bytes // 4 // 4 * 4
    parts = [x[i : min(n_floats, i + step)] for i in range(0, n_floats, step)]

    def run_two():
        two.allreduce_(x, 1.0 / world)

    def run_one():
        for p in parts:
            one.allreduce_(p, 1.0 / world)

    res = {"chunks": len(parts), "blocks": two.blocks(n_floats)}
    for name, fn in (("twophase_us", run_two), ("oneshot_chunks_us", run_one)):
        for _ in range(warmup):
            fn()
        th.cuda.synchronize(dev)
        pdist.barrier()
        times = []
        for _ in range(iters):
            e0, e1 = th.cuda.Event(enable_timing=True), th.cuda.Event(enable_timing=True)
            e0.record()
            fn()
            e1.record()
            e1.synchronize()
            times.append(e0.elapsed_time(e1) * 1e3)
        res[name] = float(np.median(times))
    res["error"] = one.error() + two.error()
    return res
