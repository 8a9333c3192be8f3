"""The device BC engine (``imitation_amd.engine.bc``; ``BC(engine=...)``).

CPU part: every eligibility rule has its own reason, ``engine="device"`` raises with it,
``engine="auto"`` falls back, a default ``BC`` never reaches the fused steps, and
``TransitionsBatchLoader.epoch_order()`` is what ``__iter__`` slices. GPU part: the engine keeps
every observable effect of ``BC.train``'s loop and is bitwise the fused steps driven by hand; it
learns; DAgger runs on it."""

import numpy as np
import pytest
import torch as th
from torch import nn

from imitation_amd.algorithms import base as algo_base
from imitation_amd.algorithms import bc
from imitation_amd.data import types
from imitation_amd.engine import bc as bc_engine
from imitation_amd.envs import spaces
from imitation_amd.ops import bc_mlp
from imitation_amd.ops.optim import FusedAdam, FusedAdamW
from imitation_amd.rl.policies import ActorCriticPolicy
from imitation_amd.util import logger

gpu = pytest.mark.gpu
HOST_LINEAR_MSE = 0.00478  # the host engine's final MSE on linear_expert_task, measured on a CPU


def _demos(head, n=100, d=4, a=2, seed=0):
    rng = np.random.default_rng(seed)
    obs = rng.standard_normal((n, d)).astype(np.float32)
    acts = rng.integers(0, a, n) if head == "cat" else rng.uniform(-1, 1, (n, a)).astype(np.float32)
    return types.TransitionsMinimal(obs=obs, acts=acts, infos=np.array([{}] * n))


def _spaces(head, d=4, a=2):
    obs_space = spaces.Box(low=-np.inf, high=np.inf, shape=(d,), dtype=np.float32)
    return obs_space, spaces.Discrete(a) if head == "cat" else spaces.Box(low=-1.0, high=1.0, shape=(a,), dtype=np.float32)


def _trainer(head="cat", seed=0, demos="default", cls=bc.BC, d=4, a=2, **kw):
    """A BC trainer from fixed seeds (policy init, ``rng`` and the loader's shuffling)."""
    th.manual_seed(seed)
    np.random.seed(seed)  # (the loader draws its shuffling seed from numpy's global generator)
    obs_space, act_space = _spaces(head, d, a)
    kw.setdefault("batch_size", 32)
    kw.setdefault("custom_logger", logger.configure(format_strs=[]))
    if demos == "default":
        demos = _demos(head, d=d, a=a)
    return cls(observation_space=obs_space, action_space=act_space, rng=np.random.default_rng(seed), demonstrations=demos,
               **kw)


# ------------------------------------------------------------------------------------ CPU
def test_every_eligibility_rule_has_its_own_reason(monkeypatch):
    """On the CPU with an explicit ``FusedAdam`` every rule but the last can be met, so each rule
    is broken on its own; the reasons are pairwise different."""
    obs_space, act_space = _spaces("cat")
    cpu = dict(device="cpu", optimizer_cls=FusedAdam)

    def policy(**kw):
        kw.setdefault("net_arch", [32, 32])
        return ActorCriticPolicy(kw.pop("obs_space", obs_space), kw.pop("act_space", act_space), lambda _: 1e-3, **kw)

    from imitation_amd.policies.base import NormalizeFeaturesExtractor

    img_space = spaces.Box(low=0, high=255, shape=(4,), dtype=np.uint8)
    seen = {}
    built = {
        "gpu": dict(),
        "accumulation": dict(minibatch_size=16),
        "batch-size": dict(batch_size=257, demos=_demos("cat", n=300)),
        "normaliser": dict(policy=policy(features_extractor_class=NormalizeFeaturesExtractor)),
        "unshared-extractor": dict(policy=policy(share_features_extractor=False)),
        "trunk-depth": dict(policy=policy(net_arch=[32, 32, 32])),
        "trunk-activation": dict(policy=policy(activation_fn=nn.ELU)),
        "width": dict(policy=policy(net_arch=dict(pi=[65, 32], vf=[8]))),
        "bucket": dict(policy=policy(net_arch=dict(pi=[32, 32], vf=[256, 256]))),
        "adamw": dict(optimizer_cls=FusedAdamW),
        "torch-adam": dict(optimizer_cls=th.optim.Adam),
        "squash": dict(head="gauss", policy=policy(act_space=_spaces("gauss")[1], squash_output=True)),
    }
    for name, kw in built.items():
        t = _trainer(**{**cpu, **kw}, engine="auto")
        assert t.engine_kind == "host"
        seen[name] = t.engine_reason
        ok, why = bc_engine.supports(t)
        assert not ok and why == t.engine_reason
    # rules of the run's surroundings, taken again on one trainer that meets every rule but the last
    t = _trainer(**cpu, engine="auto")
    assert seen["gpu"] == t.engine_reason and "GPU" in t.engine_reason

    def again(name):
        ok, why = bc_engine.supports(t)
        assert not ok
        seen[name] = why

    with monkeypatch.context() as mp:
        mp.setattr(bc_engine.pdist, "world_size", lambda: 2)
        again("world-size")
    with monkeypatch.context() as mp:
        mp.setattr(t, "observation_space", img_space)
        again("obs-space")
    with monkeypatch.context() as mp:
        mp.setattr(t.policy, "use_sde", True)
        again("use-sde")
    with monkeypatch.context() as mp:
        from imitation_amd.rl.distributions import BernoulliDistribution

        mp.setattr(t.policy, "action_dist", BernoulliDistribution(2))
        again("distribution")
    t.optimizer.param_groups[0]["weight_decay"] = 1e-2
    again("weight-decay")
    t.optimizer.param_groups[0]["weight_decay"] = 0.0
    with monkeypatch.context() as mp:
        mp.setattr(t, "optimizer", FusedAdam(list(t.policy.parameters())[1:], lr=1e-3))
        again("foreign-params")
    with monkeypatch.context() as mp:
        mp.setattr(t, "_demo_data_loader", [dict(obs=np.zeros((32, 4), np.float32), acts=np.zeros(32, np.int64))])
        again("loader")
    with monkeypatch.context() as mp:
        loader = algo_base.TransitionsBatchLoader(_demos("cat"), 32, drop_last=False)
        mp.setattr(t, "_demo_data_loader", loader)
        again("drop-last")
    ok, why = bc_engine.supports(_multibc())
    assert not ok
    seen["multibc"] = why
    assert all(seen.values()) and len(set(seen.values())) == len(seen), seen


def _multibc():
    d = 3
    return bc.MultiBC(single_agent_observation_space=spaces.Box(-10, 10, (d,)), single_agent_action_space=spaces.Discrete(2),
                      observation_overide=lambda i, o: o[:, d * i : d * i + d], action_overide=lambda i, a: a[:, i],
                      num_agents=2, rng=np.random.default_rng(0), batch_size=8, device="cpu",
                      custom_logger=logger.configure(format_strs=[]))


def test_engine_argument_semantics(monkeypatch):
    with pytest.raises(ValueError, match="'host', 'device' or 'auto'"):
        _trainer(device="cpu", engine="gpu")
    with pytest.raises(ValueError, match="engine='device' is not applicable: .*FusedAdam"):
        _trainer(device="cpu", engine="device")
    with pytest.raises(ValueError, match="engine='device' is not applicable: .*GPU"):
        _trainer(device="cpu", engine="device", optimizer_cls=FusedAdam)
    calls = []
    monkeypatch.setattr(bc_mlp, "bc_mlp_steps", lambda *a, **k: calls.append(1))
    auto = _trainer(device="cpu", engine="auto")
    assert auto.engine_kind == "host" and "FusedAdam" in auto.engine_reason
    auto.train(n_batches=3, progress_bar=False)
    default = _trainer(device="cpu")
    assert default.engine_kind == "host" and default.engine_reason == "engine='host'"
    p0 = [p.detach().clone() for p in default.policy.parameters()]
    default.train(n_batches=3, progress_bar=False)
    assert any(not th.equal(a, b.detach()) for a, b in zip(p0, default.policy.parameters()))
    assert not calls, "a host-engine BC reached the fused steps"


@pytest.mark.parametrize("shuffle,drop_last", [(True, True), (True, False), (False, True)])
def test_epoch_order_is_what_iter_slices(shuffle, drop_last):
    demos = _demos("cat", n=100)
    a = algo_base.TransitionsBatchLoader(demos, 32, shuffle=shuffle, drop_last=drop_last, seed=5)
    b = algo_base.TransitionsBatchLoader(demos, 32, shuffle=shuffle, drop_last=drop_last, seed=5)
    for _ in range(2):  # two epochs: the generators advance alike
        batches = list(a)
        order = b.epoch_order()
        assert len(order) == (96 if drop_last else 100)
        assert len(batches) == -(-len(order) // 32)
        for i, batch in enumerate(batches):
            idx = order[i * 32 : (i + 1) * 32]
            np.testing.assert_array_equal(batch["obs"], demos.obs[idx])
            np.testing.assert_array_equal(batch["acts"].numpy(), demos.acts[idx])
        assert a._rng.bit_generator.state == b._rng.bit_generator.state
    it = iter(a)  # an epoch that is begun draws its permutation at the first batch, not before
    state = a._rng.bit_generator.state
    assert a._rng.bit_generator.state == state
    next(it)
    assert (a._rng.bit_generator.state != state) == shuffle


# ------------------------------------------------------------------------------------ GPU
def _record_orders(monkeypatch):
    orders = []
    real = algo_base.TransitionsBatchLoader.epoch_order

    def spy(self):
        o = real(self)
        orders.append(np.array(o))
        return o

    monkeypatch.setattr(algo_base.TransitionsBatchLoader, "epoch_order", spy)
    return orders


def _two_calls(trainer, counts=None, on_batch_end=None):
    def epoch_end():
        counts["epoch"] += 1

    def batch_end():
        counts["batch"] += 1
        if on_batch_end is not None:
            on_batch_end()

    kw = {} if counts is None else dict(on_epoch_end=epoch_end)
    if counts is not None and "batch" in counts:
        kw["on_batch_end"] = batch_end
    trainer.train(n_batches=7, log_interval=2, progress_bar=False, **kw)
    trainer.train(n_epochs=2, progress_bar=False, **kw)


@gpu
@pytest.mark.parametrize("head", ["cat", "gauss"])
def test_loop_fidelity(head, monkeypatch):
    """100 rows at B = 32 (three batches per epoch), ``train(n_batches=7, log_interval=2)`` then
    ``train(n_epochs=2)``: the device engine is bitwise ``bc_mlp_steps`` driven by hand with the
    loader's orders, logs those metric rows, draws the batch ids a host-engine run draws and calls
    the callbacks as often as the host engine does."""
    kw = dict(device="cuda", l2_weight=3e-5, optimizer_kwargs=dict(lr=1e-3))
    orders = _record_orders(monkeypatch)
    logged = []
    real_log = bc.BCLogger.log_batch

    def log_spy(self, batch_num, batch_size, num_samples_so_far, training_metrics, rollout_stats):
        logged.append((batch_num, batch_size, num_samples_so_far, self._current_epoch,
                       th.stack([getattr(training_metrics, k).reshape(()) for k in bc_mlp.BC_METRICS]).cpu()))
        return real_log(self, batch_num, batch_size, num_samples_so_far, training_metrics, rollout_stats)

    monkeypatch.setattr(bc.BCLogger, "log_batch", log_spy)
    dev = _trainer(head, engine="device", **kw)
    assert dev.engine_kind == "device" and dev.engine_reason == ""
    counts = dict(epoch=0)
    _two_calls(dev, counts)
    dev_orders, dev_logged = list(orders), list(logged)
    assert [len(o) for o in dev_orders] == [96] * 5
    assert counts["epoch"] == 2 + 2
    # launches: call 1 ends one at the logged batches 0, 2, 4, 6 and at each epoch's end; call 2
    # logs batch 0 and runs the rest of each epoch in one launch
    assert dev._engine.n_launches == 5 + 3

    # by hand: the same seeds, the fused steps one by one on the loader's orders
    del orders[:], logged[:]
    hand = _trainer(head, engine="host", **kw)
    L = bc_mlp.BCMlpLayout.from_policy(hand.policy, hand.optimizer)
    f = hand.optimizer._flat[0]
    obs = th.as_tensor(_demos(head).obs, device="cuda")
    acts = th.as_tensor(_demos(head).acts, device="cuda")
    rows = []
    for order, nb in zip(dev_orders, [3, 3, 1, 3, 3]):
        for b in range(nb):
            ids = th.as_tensor(order[b * 32 : (b + 1) * 32], device="cuda").reshape(1, 32)
            rows.append(bc_mlp.bc_mlp_steps(obs, acts, ids, f["flat"], None, f["m"], f["v"], f["step"], L, lr=1e-3,
                                            ent_weight=1e-3, l2_weight=3e-5)[0].cpu())
    g = dev.optimizer._flat[0]
    for key in ("flat", "m", "v", "step", "grad"):
        assert th.equal(f[key], g[key]), key
    assert float(g["step"]) == 13.0 and not bool(g["grad"].any())
    assert [(x[0], x[1], x[2], x[3]) for x in dev_logged] == [(0, 32, 32, 0), (2, 32, 96, 0), (4, 32, 160, 1),
                                                              (6, 32, 224, 2), (0, 32, 32, 0)]
    for x, i in zip(dev_logged, [0, 2, 4, 6, 7]):
        assert th.equal(x[4], rows[i]), i

    # the host engine from the same seeds: the same batch ids, as many callbacks
    del orders[:], logged[:]
    host = _trainer(head, engine="host", **kw)
    h_counts = dict(epoch=0, batch=0)
    _two_calls(host, h_counts)
    assert len(orders) == 5 and all(np.array_equal(a, b) for a, b in zip(orders, dev_orders))
    assert [x[:4] for x in logged] == [x[:4] for x in dev_logged]

    # with on_batch_end every launch is one step and the policy is already updated at each call
    dev2 = _trainer(head, engine="device", **kw)
    d_counts = dict(epoch=0, batch=0)
    snaps = []
    _two_calls(dev2, d_counts, on_batch_end=lambda: snaps.append(dev2.optimizer._flat[0]["flat"].clone()))
    assert d_counts == h_counts == dict(epoch=4, batch=13)
    assert dev2._engine.n_launches == 13
    assert all(not th.equal(a, b) for a, b in zip(snaps, snaps[1:]))
    assert th.equal(snaps[-1], g["flat"])


@gpu
def test_device_engine_learns_the_sign_rule():
    """The sign-rule task of ``test_multibc_trains_on_agent_concatenated_batches`` with one agent."""
    rng = np.random.default_rng(0)
    obs = rng.standard_normal((512, 3)).astype(np.float32)
    acts = (obs[:, 0] > 0).astype(np.int64)
    demos = types.TransitionsMinimal(obs=obs, acts=acts, infos=np.array([{}] * 512))
    t = _trainer("cat", d=3, demos=demos, device="cuda", engine="device", batch_size=64, optimizer_kwargs=dict(lr=3e-3))
    t.train(n_epochs=15, progress_bar=False, log_interval=10**9)
    assert t.engine_kind == "device"
    pred, _ = t.policy.predict(obs, deterministic=True)
    assert (pred == acts).mean() > 0.9


def linear_expert_task(device, engine):
    """BC on a linear expert ``a = M obs`` (6 -> 3, 512 rows, B = 64, lr 3e-3, 30 epochs): the
    final MSE of the deterministic action."""
    rng = np.random.default_rng(1)
    obs = rng.standard_normal((512, 6)).astype(np.float32)
    M = (rng.standard_normal((6, 3)) * 0.3).astype(np.float32)
    acts = obs @ M
    demos = types.TransitionsMinimal(obs=obs, acts=acts, infos=np.array([{}] * 512))
    t = _trainer("gauss", d=6, a=3, demos=demos, device=device, engine=engine, batch_size=64,
                 optimizer_kwargs=dict(lr=3e-3))
    t.train(n_epochs=30, progress_bar=False, log_interval=10**9)
    with th.no_grad():
        mean = t.policy.get_distribution(th.tensor(obs, device=t.policy.device)).mean_actions
    return t, float(((mean.cpu() - th.as_tensor(acts)) ** 2).mean())


@gpu
def test_device_engine_learns_a_linear_expert():
    """The bar is the host engine on the CPU from the same seeds, measured before this test was
    written: final MSE 0.00478 (``linear_expert_task("cpu", "host")``). The device engine's final MSE must be at most twice
    that (the margin covers fp32 summation order under Adam)."""
    t, mse = linear_expert_task("cuda", "device")
    assert t.engine_kind == "device"
    print(f"linear expert: device MSE {mse:.6f}, host (CPU) MSE {HOST_LINEAR_MSE:.6f}")
    assert mse <= 2 * HOST_LINEAR_MSE


@gpu
def test_dagger_runs_on_the_device_engine(tmp_path):
    from imitation_amd.algorithms import dagger
    from imitation_amd.policies.base import FeedForward32Policy
    from imitation_amd.util.util import make_vec_env

    th.manual_seed(0)
    np.random.seed(0)
    venv = make_vec_env("seals/CartPole-v0", rng=np.random.default_rng(0), n_envs=2)
    expert = FeedForward32Policy(venv.observation_space, venv.action_space, lambda _: 1e-3).cuda()
    log = logger.configure(str(tmp_path / "log"), format_strs=[])
    bct = bc.BC(observation_space=venv.observation_space, action_space=venv.action_space, rng=np.random.default_rng(0),
                batch_size=32, device="cuda", custom_logger=log, engine="device")
    assert bct.engine_kind == "device"
    tr = dagger.SimpleDAggerTrainer(venv=venv, scratch_dir=tmp_path / "scratch", expert_policy=expert,
                                    rng=np.random.default_rng(0), bc_trainer=bct, custom_logger=log)
    assert tr.collector_kind == "host"  # ('auto' keeps host demonstrations for the device BC engine)
    kinds = []
    p0 = bct.optimizer._flat[0]["flat"].clone()
    tr.train(2 * 600, rollout_round_min_episodes=1, rollout_round_min_timesteps=600,
             bc_train_kwargs=dict(n_epochs=1, progress_bar=False, log_interval=10**9,
                                  on_epoch_end=lambda: kinds.append(bct.engine_kind)))
    assert tr.round_num >= 2 and kinds and set(kinds) == {"device"}
    assert bct.engine_kind == "device" and bct._engine.n_launches >= 2
    assert not th.equal(p0, bct.optimizer._flat[0]["flat"])
