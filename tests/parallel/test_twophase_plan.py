"""Host-side planning of the two-phase all-reduce (no GPU): the Python mirror of the kernel's
shard bounds, the reduction ranges of the graph-resident DP BC step with and without the large
communicator, and ``get_large`` without a process group."""

import types

import pytest
import torch as th

from imitation_amd.algorithms import bc
from imitation_amd.parallel import oneshot


@pytest.mark.parametrize("world", range(1, 9))
def test_shard_mirror_tiles_every_slice(world):
    """Over ``r`` the shards cover ``[v0, v1)`` exactly once, in rank order, slices shorter than
    ``world`` included (some shards are then empty); sizes differ by at most one vector."""
    for v0 in (0, 5, 256, 3291 * 7):
        for length in list(range(0, 20)) + [255, 256, 257, 3291, 32768]:
            v1 = v0 + length
            pos, lens = v0, []
            for r in range(world):
                lo, hi = oneshot.twophase_shard(v0, v1, world, r)
                assert lo == pos and lo <= hi <= v1
                lens.append(hi - lo)
                pos = hi
            assert pos == v1
            assert max(lens) - min(lens) <= 1
            if length < world:
                assert lens.count(0) == world - length


FC_OFF, FC_N, TAIL = 77984, 1_605_632, 1000


def _runner(stage_bytes, large):
    flat = th.zeros(FC_OFF + FC_N + TAIL)
    runner = bc._DeviceEpochRunner.__new__(bc._DeviceEpochRunner)
    runner.trainer = types.SimpleNamespace(optimizer=types.SimpleNamespace(flat_grads=[flat]))
    runner._comm = types.SimpleNamespace(stage_bytes=stage_bytes)
    if large is not None:
        runner._large = large
    runner._f = types.SimpleNamespace(g_lin=[flat[FC_OFF : FC_OFF + FC_N]])
    return runner, flat


def _spans(parts, flat):
    return [((t.data_ptr() - flat.data_ptr()) // 4, t.numel()) for t in parts]


def test_dp_ranges_send_the_fc_range_as_one_part_to_the_large_communicator():
    large = types.SimpleNamespace(stage_bytes=(FC_OFF + FC_N + TAIL) * 4)
    runner, flat = _runner(1 << 20, large)
    fc, rest = runner._dp_ranges()
    assert _spans(fc, flat) == [(FC_OFF, FC_N)]  # ONE early part: the whole FC weight gradient
    step = (1 << 20) // 4
    assert all(n <= step for _, n in _spans(rest, flat))
    pos = 0
    for o, n in sorted(_spans(fc + rest, flat)):  # the bucket is covered exactly once
        assert o == pos and n > 0
        pos += n
    assert pos == flat.numel()


@pytest.mark.parametrize("case", ["absent", "none", "slot_big_enough", "large_too_small"])
def test_dp_ranges_keep_the_one_shot_chunks_otherwise(case):
    big = types.SimpleNamespace(stage_bytes=(FC_OFF + FC_N + TAIL) * 4)
    stage, large = {"absent": (1 << 20, None), "none": (1 << 20, None), "slot_big_enough": (8 << 20, big),
                    "large_too_small": (1 << 20, types.SimpleNamespace(stage_bytes=1 << 20))}[case]
    runner, flat = _runner(stage, large)
    if case == "none":
        runner._large = None
    fc, rest = runner._dp_ranges()
    ref, ref_flat = _runner(stage, None)  # today's chunking
    step = stage // 4 // 4 * 4
    exp_fc = [(i, min(FC_OFF + FC_N, i + step) - i) for i in range(FC_OFF, FC_OFF + FC_N, step)]
    assert _spans(fc, flat) == exp_fc
    assert _spans(fc, flat) == _spans(ref._dp_ranges()[0], ref_flat)
    assert _spans(rest, flat) == _spans(ref._dp_ranges()[1], ref_flat)
    assert all(n * 4 <= stage for _, n in _spans(fc + rest, flat))
    assert len(fc) == (7 if stage == 1 << 20 else 1)


def test_get_large_is_none_without_a_process_group():
    oneshot.reset()
    try:
        assert oneshot.get_large(6 << 20) is None
        assert oneshot._LARGE is None
    finally:
        oneshot.reset()
