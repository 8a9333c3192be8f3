"""Two-phase IPC all-reduce (``twophase_allreduce_kernel`` in csrc/kernels/comm.hip,
``TwoPhaseComm`` / ``get_large`` in parallel/oneshot.py): ranks share one GPU over a gloo
bootstrap group with ``IMITATION_AMD_ONESHOT=1``. The oracle is the numpy rank-order sum
(``x_r * scale`` accumulated in the element type in rank order); every comparison is bitwise.

The slot is deliberately small -- 512 KiB, so a block slice is ``PER`` = 256 vectors at 128
blocks -- and the block / shard edges are reached with small arrays."""

import numpy as np
import pytest

from imitation_amd.testing import twophase_workers as TW
from imitation_amd.testing.distributed import run_ranks

SLOT = 512 << 10
MAX_BLOCKS = 128
PER = SLOT // 16 // MAX_BLOCKS  # vectors per block slice
assert PER == 256


@pytest.fixture
def oneshot_env(monkeypatch):
    monkeypatch.setenv("IMITATION_AMD_DIST_BACKEND", "gloo")
    monkeypatch.setenv("IMITATION_AMD_ONESHOT", "1")


def _sizes(world):
    """fp32 sizes: 1, 7, fewer vectors than ranks (empty shards) plus a tail, exactly one block, a
    second block holding one vector, three blocks plus a tail, the full slot."""
    return [1, 7, 4 * (world - 1) + 1, 4 * PER, 4 * PER + 4, 4 * 3 * PER + 3, SLOT // 4]


def _f64_sizes(world):
    return [(n + 1) // 2 for n in _sizes(world)[:5]]  # the first five, halved: the same bytes


def _expected(world, n, scale, seed, extra=0, f64=False):
    acc = None
    for r in range(world):
        x = np.random.default_rng(seed * 100 + r * 7 + n + extra).normal(size=n)
        x = x * scale if f64 else x.astype(np.float32) * np.float32(scale)
        acc = x if acc is None else (acc + x if f64 else (acc + x).astype(np.float32))
    return acc


@pytest.mark.gpu
@pytest.mark.parametrize("world", [2, 3, 4])
def test_twophase_matches_rank_order_sum(world, oneshot_env):
    sizes, f64_sizes, scale, seed = _sizes(world), _f64_sizes(world), 1.0 / world, 3
    out = run_ranks(TW.twophase_worker, world, SLOT, sizes, f64_sizes, scale, seed, timeout=240)
    for r in range(world):
        assert out[r]["error"] == 0
        assert out[r]["blocks"] == [1, 1, 1, 1, 2, 4, MAX_BLOCKS]
        for n, got in zip(sizes, out[r]["eager"]):
            assert got.dtype == np.float32
            np.testing.assert_array_equal(got, _expected(world, n, scale, seed))
        for n, got in zip(f64_sizes, out[r]["f64"]):
            assert got.dtype == np.float64
            np.testing.assert_array_equal(got, _expected(world, n, scale, seed, 5, f64=True))
        assert len(out[r]["graph"]) == 3
        for rep, got in enumerate(out[r]["graph"]):
            np.testing.assert_array_equal(got, _expected(world, SLOT // 4, scale, seed, 1000 + rep))


def _slices(world):
    """The (v0, v1) block slices the sizes of the test above reach (fp32 and fp64 elements)."""
    seen = set()
    for epv, sizes in ((4, _sizes(world)), (2, _f64_sizes(world))):
        for n in sizes:
            nv = n // epv  # whole vectors; the launch covers ceil(n / epv) of them
            for b in range(max(1, -(-(-(-n // epv)) // PER))):  # = ceil(ceil(n / epv) / PER)
                v0 = min(nv, b * PER)
                seen.add((v0, min(nv, v0 + PER)))
    return sorted(seen)


@pytest.mark.gpu
def test_twophase_shard_bounds_match_python():
    """The kernel's shard bounds (through the binding) equal the Python mirror, and over ``r``
    the shards tile the slice exactly and in order."""
    from imitation_amd import _native
    from imitation_amd.parallel import oneshot

    C = _native.load()
    n_checked = 0
    for world in (2, 3, 4):
        for v0, v1 in _slices(world):
            pos = v0
            for r in range(world):
                lo, hi = C.twophase_shard(v0, v1, world, r)
                assert (lo, hi) == tuple(oneshot.twophase_shard(v0, v1, world, r))
                assert lo == pos and hi >= lo
                pos = hi
                n_checked += 1
            assert pos == v1
    assert n_checked > 50
    assert C.twophase_region_bytes(SLOT) >= 2 * SLOT
    assert C.twophase_blocks(SLOT // 4, SLOT) == MAX_BLOCKS and C.twophase_blocks(1, SLOT) == 1


@pytest.mark.gpu
def test_twophase_uneven_arrival(oneshot_env):
    """60 reductions, each on the one-shot or the two-phase communicator and of a size of the
    first test, with random per-rank host sleeps and GPU busy work in front of each: every word
    exact (small integers plus halves: any order is exact), neither error word raised."""
    out = run_ranks(TW.twophase_stress_worker, 4, SLOT, _sizes(4), 60, 11, timeout=240)
    for o in out:
        assert o["bad_words"] == 0 and o["error_oneshot"] == 0 and o["error_twophase"] == 0, o
        assert min(o["picks"]) > 0  # both communicators were exercised


@pytest.mark.gpu
def test_twophase_block_count_changes_in_one_graph(oneshot_env):
    """One graph holding back-to-back two-phase reductions of 1, 3, 128 and 1 blocks, replayed 8
    times under rank-skewed load: zero wrong words (single staging / result areas, fixed block
    slices, the two waits ordering consecutive calls)."""
    out = run_ranks(TW.twophase_block_change_worker, 2, SLOT, 8, 5, timeout=240)
    for r in range(2):
        assert out[r]["blocks"] == [1, 3, MAX_BLOCKS, 1]
        assert out[r]["bad_words"] == 0 and out[r]["error"] == 0


@pytest.mark.gpu
def test_twophase_bounded_wait(oneshot_env):
    """A peer that never issues the call: the kernel ends by itself with all-NaN output and the
    error word raised; ``check(blocking=True)`` raises and clears it."""
    out = run_ranks(TW.twophase_timeout_worker, 2, SLOT, 0.25, timeout=240)
    assert out[0]["all_nan"] and out[0]["error"] == 1
    assert out[0]["raised"] and out[0]["error_after"] == 0


@pytest.mark.gpu
def test_bc_dp_epoch_graphs_on_twophase_are_bitwise(monkeypatch):
    """Graph-resident DP BC with the FC gradient range on the two-phase kernel (default 1 MiB
    one-shot slot) is bitwise the all-one-shot epoch runner and the per-minibatch
    ``_DPFusedStep`` (8 MiB slot): parameters, Adam moments and every logged BC metric, on all
    ranks of all three runs."""
    monkeypatch.setenv("IMITATION_AMD_DIST_BACKEND", "gloo")
    monkeypatch.setenv("IMITATION_AMD_ONESHOT", "1")
    monkeypatch.delenv("IMITATION_AMD_ONESHOT_MAX_BYTES", raising=False)
    two = run_ranks(TW.bc_dp_epoch_calls_worker, 2, "1", timeout=240)
    monkeypatch.setenv("IMITATION_AMD_ONESHOT_MAX_BYTES", str(8 << 20))
    one = run_ranks(TW.bc_dp_epoch_calls_worker, 2, "1", timeout=240)
    per_mb = run_ranks(TW.bc_dp_epoch_calls_worker, 2, "0", timeout=240)
    assert all(o["epoch_runner"] and o["twophase_calls"] > 0 and o["twophase_error"] == 0 for o in two)
    assert all(o["epoch_runner"] and o["twophase_calls"] == 0 and o["oneshot_calls"] > 0 for o in one)
    assert all(not o["epoch_runner"] and o["twophase_calls"] == 0 and o["dp_fused_replays"] > 0 for o in per_mb)
    ref = two[0]
    for o in two + one + per_mb:
        assert len(o["params"]) == len(ref["params"])
        for a, b in zip(o["params"], ref["params"]):
            np.testing.assert_array_equal(a, b)
        np.testing.assert_array_equal(o["m"], ref["m"])
        np.testing.assert_array_equal(o["v"], ref["v"])
    for r in range(2):
        assert len(two[r]["recorded"]) > 0
        for other in (one, per_mb):
            assert [s for s, _ in two[r]["recorded"]] == [s for s, _ in other[r]["recorded"]]
            for (_, a), (_, b) in zip(two[r]["recorded"], other[r]["recorded"]):
                assert a == b
