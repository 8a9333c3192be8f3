"""Launch sequence of the fused discriminator drivers of DeviceGAIL and DeviceAIRL (CPU).

The real unbound methods of the two engines run on a stand-in with a recording plan, a recording
demo sampler and recording collectives. The expected sequences are written out here, not derived
from the code under test: they are the order the engines issued their launches, collectives and
index draws in before GAIL and AIRL shared one driver, and a reordering changes bits or opens a
race. Two minibatches per batch: the smallest case that shows the loop order."""

import inspect
import types

import pytest
import torch as th
from torch import nn

from imitation_amd.engine.airl import DeviceAIRL
from imitation_amd.engine.gail import DeviceEngineMixin, DeviceGAIL
from imitation_amd.parallel import dist as pdist

MB = 4
B = 2 * MB
N_REPLAY = 100
LR, BETA1, BETA2 = 3e-4, 0.9, 0.999
DRAWS = [("next_indices", ()), ("randint", (0, N_REPLAY, (B,)))]


def scalars(t: float):
    return LR / (1 - BETA1**t), (1 - BETA2**t) ** 0.5


class E:
    """Expert indices of draw ``i`` (equal by ``i``)."""

    def __init__(self, i, log=None):
        self.i, self.log = i, log

    def record_stream(self, stream):
        self.log.append(("record_stream", (self, stream)))

    def __eq__(self, other):
        return isinstance(other, E) and other.i == self.i

    def __repr__(self):
        return f"E({self.i})"


class _Sampler:
    def __init__(self, log):
        self.log, self.n = log, 0

    def next_indices(self):
        self.log.append(("next_indices", ()))
        self.n += 1
        return E(self.n - 1, self.log)


class _Plan:
    n_minibatches = B // MB

    def __init__(self, log, engine):
        self.log, self.engine, self.disc_steps_seen = log, engine, []

    def __getattr__(self, name):
        def call(*args):
            self.log.append((name, args))
            self.disc_steps_seen.append(self.engine._disc_step)

        return call


def _stand_in(engine_cls, monkeypatch, world=1, sync=True, training=True):
    """``engine_cls``'s own functions and the mixin's on a plain class; returns (engine, log)."""
    ns = {}
    for c in (DeviceEngineMixin, engine_cls):
        ns.update({k: v for k, v in vars(c).items() if inspect.isfunction(v) and not k.startswith("__")})
    e = type("Engine", (), ns)()
    log = []
    params = [nn.Parameter(th.zeros(3, 2)), nn.Parameter(th.zeros(3))]
    e._disc_opt = th.optim.Adam(params, lr=LR, betas=(BETA1, BETA2))
    e._rflat = types.SimpleNamespace(params=params, offsets=[0, 6], n=9)
    e._r_m, e._r_v = th.zeros(9), th.zeros(9)
    e._dev = "cpu"
    e.demo_batch_size, e.demo_minibatch_size = B, MB
    e._gen_dev = types.SimpleNamespace(size=lambda: N_REPLAY)
    e._endless_expert_iterator = _Sampler(log)
    e._disc_plan = _Plan(log, e)
    e._disc_stats = ["stats0", "stats1", "stats2"]
    e._disc_ws = {"sums": "sums", "grads": "grads"}
    e._disc_step = 0
    norm = types.SimpleNamespace(training=training)
    e.pol_norm = e._rnorm = e._bnorm = e._pnorm = norm
    monkeypatch.setattr(pdist, "world_size", lambda: world)
    monkeypatch.setattr(pdist, "norm_sync_active", lambda: sync and world > 1)
    monkeypatch.setattr(pdist, "allreduce_sum_", lambda t: log.append(("allreduce_sum_", (t,))))
    monkeypatch.setattr(pdist, "allreduce_grads_flat", lambda t: log.append(("allreduce_grads_flat", (t,))))
    monkeypatch.setattr(th, "randint", lambda lo, hi, shape, device=None: (log.append(("randint", (lo, hi, shape))),
                                                                          "g")[1])
    monkeypatch.setattr(th.cuda, "current_stream", lambda dev=None: "stream")
    return e, log


def _take(log):
    out = list(log)
    del log[:]
    return out


def _opt_steps(e):
    return [float(e._disc_opt.state[p]["step"]) for p in e._rflat.params] + [float(e._disc_step)]


def _dp_update(i, slot, merges, norm, ds=None, apply=True, world=2):
    """The data-parallel order of one update: ``norm`` is None (no launch), "sync" or "local";
    ``ds``: GAIL's deferred slot of the first minibatch (None: no slot argument)."""
    seq = []
    for k in range(2):
        tail = () if ds is None else (ds + k if ds >= 0 else -1,)
        seq.append(("gather", (k, E(i), "g")))
        if norm == "sync":
            seq += [("norm", (1, 0) + merges), ("allreduce_sum_", ("sums",)), ("norm", (2, 4 * MB) + merges + tail)]
        elif norm == "local":
            seq.append(("norm", (0, 0) + merges + tail))
        seq.append(("fwd_bwd", (k,)))
    seq.append(("adam", (1, 0, 0.0, 1.0, f"stats{slot}")))
    if world > 1:
        seq.append(("allreduce_grads_flat", ("grads",)))
    if apply:
        seq.append(("adam", (0, 1) + scalars(float(i + 1)) + (None,)))
    return seq


# ---------------------------------------------------------------------------------------- GAIL
def test_gail_single_rank_is_one_update_launch(monkeypatch):
    e, log = _stand_in(DeviceGAIL, monkeypatch)
    for t, (slot, defer, base) in enumerate([(0, False, -1), (1, True, 2), (2, True, 4)], start=1):
        e._fused_disc_update(slot, defer_pol=defer)
        assert _take(log) == DRAWS + [
            ("update", (E(t - 1), "g") + scalars(float(t)) + (True, True, f"stats{slot}", base))]
        assert _opt_steps(e) == [t, t, t]  # t = 3 after three runs: the bump reaches every step counter


def test_gail_frozen_norms_do_not_merge_or_defer(monkeypatch):
    e, log = _stand_in(DeviceGAIL, monkeypatch, training=False)
    e._fused_disc_update(1, defer_pol=True)
    assert _take(log) == DRAWS + [("update", (E(0), "g") + scalars(1.0) + (False, False, "stats1", -1))]
    e._rnorm = types.SimpleNamespace(training=True)  # reward norm merges, nothing to defer
    e._fused_disc_update(1, defer_pol=True)
    assert _take(log) == DRAWS + [("update", (E(1), "g") + scalars(2.0) + (True, False, "stats1", -1))]


def test_gail_data_parallel_order(monkeypatch):
    e, log = _stand_in(DeviceGAIL, monkeypatch, world=2)
    e._fused_disc_update(1, defer_pol=True)
    assert _take(log) == DRAWS + _dp_update(0, 1, (True, True), "sync", ds=2)
    e._fused_disc_update(0)
    assert _take(log) == DRAWS + _dp_update(1, 0, (True, True), "sync", ds=-1)
    assert _opt_steps(e) == [2, 2, 2]


def test_gail_data_parallel_without_norm_sync(monkeypatch):
    e, log = _stand_in(DeviceGAIL, monkeypatch, world=2, sync=False)
    e._fused_disc_update(1, defer_pol=True)
    assert _take(log) == DRAWS + _dp_update(0, 1, (True, True), "local", ds=2)


def test_gail_data_parallel_nothing_merging_skips_the_norm_launch(monkeypatch):
    e, log = _stand_in(DeviceGAIL, monkeypatch, world=2, training=False)
    e._fused_disc_update(0, defer_pol=True)
    assert _take(log) == DRAWS + _dp_update(0, 0, (False, False), None)


# ---------------------------------------------------------------------------------------- AIRL
def test_airl_single_rank_is_one_update_launch(monkeypatch):
    e, log = _stand_in(DeviceAIRL, monkeypatch)
    for t in (1, 2, 3):
        e._fused_disc_update(t - 1)
        assert _take(log) == DRAWS + [("update", (E(t - 1), "g") + scalars(float(t)) + (True, True, True, f"stats{t - 1}"))]
        assert _opt_steps(e) == [t, t, t]


@pytest.mark.parametrize("training", [True, False])
def test_airl_data_parallel_order_always_launches_norm(monkeypatch, training):
    e, log = _stand_in(DeviceAIRL, monkeypatch, world=2, training=training)
    e._fused_disc_update(1)
    assert _take(log) == DRAWS + _dp_update(0, 1, (training,) * 3, "sync")
    assert _opt_steps(e) == [1, 1, 1]
    monkeypatch.setattr(pdist, "norm_sync_active", lambda: False)
    e._fused_disc_update(2)
    assert _take(log) == DRAWS + _dp_update(1, 2, (training,) * 3, "local")


@pytest.mark.parametrize("world", [1, 2])
def test_airl_apply_false_stops_after_the_gradient(monkeypatch, world):
    e, log = _stand_in(DeviceAIRL, monkeypatch, world=world)
    e._fused_disc_update(0, apply=False)
    assert _take(log) == DRAWS + _dp_update(0, 0, (True,) * 3, "sync" if world > 1 else "local", apply=False, world=world)
    assert _opt_steps(e) == [0, 0, 0]  # no step bump


def test_airl_given_indices_are_not_drawn(monkeypatch):
    e, log = _stand_in(DeviceAIRL, monkeypatch)
    e._fused_disc_update(0, e_idx=E(7), g_idx="mine")
    assert _take(log) == [("update", (E(7), "mine") + scalars(1.0) + (True, True, True, "stats0"))]
    e._fused_disc_update(0, g_idx="mine")  # each on its own
    assert _take(log) == [("next_indices", ()), ("update", (E(0), "mine") + scalars(2.0) + (True, True, True, "stats0"))]


def _staged(log):
    """The log without the ``record_stream`` marks, after checking them: every drawn expert index
    block is kept alive for the current stream before the first launch that reads it."""
    for j, (name, args) in enumerate(log):
        if name in ("stage", "stage_part"):
            e_idx = next(a for a in args if isinstance(a, E))
            assert ("record_stream", (e_idx, "stream")) in log[:j], (name, args)
    return [entry for entry in log if entry[0] != "record_stream"]


@pytest.mark.parametrize("defer_q", [False, True])
def test_airl_stage_single_rank(monkeypatch, defer_q):
    e, log = _stand_in(DeviceAIRL, monkeypatch)
    e._fused_disc_update(0)  # staged scalars start from the optimizer's step: t0 = 1
    _take(log)
    scal = e._stage_disc_updates(2, defer_q=defer_q)
    want = [("reserve", (2,))]
    for i in range(2):
        want += DRAWS + [("stage", (i, E(1 + i), "g", True, True, True, defer_q))]
    assert _staged(_take(log)) == want
    assert scal == [scalars(2.0), scalars(3.0)]
    assert _opt_steps(e) == [1, 1, 1]  # staging applies nothing
    e._merge_deferred_q(2)
    e._merge_deferred_q(2)  # merged once
    assert _take(log) == ([("q_merge", (2, 2 * MB))] if defer_q else [])


def test_airl_stage_data_parallel(monkeypatch):
    e, log = _stand_in(DeviceAIRL, monkeypatch, world=2)
    scal = e._stage_disc_updates(2, defer_q=True)
    want = [("reserve", (2,))]
    for i in range(2):
        want += DRAWS
        for k in range(2):
            want += [("stage_part", (i, k, E(i), "g", 1, 0, True, True, True)), ("allreduce_sum_", ("sums",)),
                     ("stage_part", (i, k, E(i), "g", 2, 4 * MB, True, True, True, True))]
    assert _staged(_take(log)) == want
    assert scal == [scalars(1.0), scalars(2.0)]
    e._merge_deferred_q(2)  # the merged moments are the whole group's rows
    assert _take(log) == [("q_merge", (2, 4 * MB))]
    monkeypatch.setattr(pdist, "norm_sync_active", lambda: False)  # no moments to reduce: whole stages
    e._stage_disc_updates(1)
    assert _staged(_take(log)) == [("reserve", (1,))] + DRAWS + [("stage", (0, E(2), "g", True, True, True, False))]


def test_airl_stage_defers_only_a_merging_policy_norm(monkeypatch):
    e, log = _stand_in(DeviceAIRL, monkeypatch)
    e.pol_norm = types.SimpleNamespace(training=False)
    e._stage_disc_updates(1, defer_q=True)
    assert _staged(_take(log)) == [("reserve", (1,))] + DRAWS + [("stage", (0, E(0), "g", True, True, False, False))]
    e._merge_deferred_q(1)
    assert _take(log) == []


@pytest.mark.parametrize("world", [1, 2])
def test_airl_apply_staged_updates(monkeypatch, world):
    e, log = _stand_in(DeviceAIRL, monkeypatch, world=world)
    monkeypatch.setattr(pdist, "norm_sync_active", lambda: False)
    scal, steps = e._stage_disc_updates(2), []
    assert scal == [scalars(1.0), scalars(2.0)]
    _take(log)
    del e._disc_plan.disc_steps_seen[:]
    e._apply_disc_updates(scal, steps)
    want = []
    for i in range(2):
        if world == 1:
            want.append(("apply", (i,) + scal[i] + (f"stats{i}",)))
        else:
            want += [("apply_grads", (i, f"stats{i}")), ("allreduce_grads_flat", ("grads",)),
                     ("adam", (0, 1) + scal[i] + (None,))]
    assert _take(log) == want
    assert steps == [1, 2] and _opt_steps(e) == [2, 2, 2]
    # the bump follows each update's launches
    assert e._disc_plan.disc_steps_seen == ([0, 1] if world == 1 else [0, 0, 1, 1])
