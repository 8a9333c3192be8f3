"""``DeviceDQN`` (``engine/dqn.py``): the host loop's schedule, the replay ring, logging and
learning with acting, env stepping and replay writes in one launch per ``train_freq`` chunk."""

import numpy as np
import pytest
import torch as th

from imitation_amd.algorithms import sqil
from imitation_amd.data import rollout
from imitation_amd.engine.dqn import DeviceDQN
from imitation_amd.ops import dqn as td
from imitation_amd.rl import dqn as dqn_mod
from imitation_amd.rl import evaluation
from imitation_amd.rl.callbacks import BaseCallback
from imitation_amd.rl.dqn import DQN
from imitation_amd.testing import reward_improvement

pytestmark = pytest.mark.gpu

# seed of the learning test: the first of 42, 43, ... at which the host control passes on the card
LEARNING_SEED = 42
STEPS = 203
KW = dict(learning_starts=50, target_update_interval=40, exploration_fraction=0.5, batch_size=32, seed=0, device="cuda")


def _venv(n_envs=1, env_id="seals/CartPole-v0"):
    from imitation_amd.data.wrappers import RolloutInfoWrapper
    from imitation_amd.util.util import make_vec_env

    return make_vec_env(env_id, rng=np.random.default_rng(0), n_envs=n_envs,
                        post_wrappers=[lambda e, _: RolloutInfoWrapper(e)])


@pytest.fixture
def demos(cartpole_expert_trajectories):
    return rollout.flatten_trajectories(cartpole_expert_trajectories[:8])


def _build(kind, n_envs, device_engine, demos, env_id="seals/CartPole-v0", **kw):
    """(algo, engine or None, learn(steps, **learn kwargs))."""
    kwargs = dict(KW)
    kwargs.update(kw)
    venv = _venv(n_envs, env_id)
    if kind == "dqn":
        algo = DQN("MlpPolicy", venv, **kwargs)
        eng = DeviceDQN(algo, venv) if device_engine else None
        learner = eng if device_engine else algo
        return algo, eng, lambda steps, **k: learner.learn(steps, **k)
    model = sqil.SQIL(venv=venv, demonstrations=demos, policy="MlpPolicy", rl_algo_class=DQN, rl_kwargs=kwargs,
                      engine="device" if device_engine else "host")
    assert model.engine_kind == ("device" if device_engine else "host")
    return model.rl_algo, model._engine, lambda steps, **k: model.train(total_timesteps=steps, **k)


class _Mirror0(BaseCallback):
    """Clones the engine's env block as training starts."""

    def __init__(self, eng):
        super().__init__()
        self.eng, self.env0 = eng, None

    def _on_training_start(self) -> None:
        self.env0 = {k: (v.clone() if isinstance(v, th.Tensor) else v) for k, v in self.eng._env_tensors().items()}

    def _on_step(self) -> bool:
        return True


@pytest.mark.parametrize("kind,n_envs", [("dqn", 1), ("dqn", 4), ("sqil", 1), ("sqil", 4)])
def test_same_schedule_as_the_host_loop(kind, n_envs, demos, monkeypatch):
    calls = {"n": 0}
    real = dqn_mod.polyak_update

    def counted(*a, **k):
        calls["n"] += 1
        return real(*a, **k)

    monkeypatch.setattr(dqn_mod, "polyak_update", counted)
    host, _, host_learn = _build(kind, n_envs, False, demos)
    host_learn(STEPS)
    host_syncs = calls["n"] // 2  # (parameters, then buffers)

    algo, eng, learn = _build(kind, n_envs, True, demos)
    p0 = [p.detach().clone() for p in algo.q_net.parameters()]
    snap = {}
    real_sync = eng._sync_target

    def sync():
        due = eng._syncs_due
        real_sync()
        if due:
            snap["online"] = algo.policy.optimizer._flat[0]["flat"].clone()

    monkeypatch.setattr(eng, "_sync_target", sync)
    learn(STEPS)
    for name in ("num_timesteps", "_n_updates", "_n_calls", "exploration_rate"):
        assert getattr(algo, name) == getattr(host, name), name
    assert (algo.replay_buffer.pos, algo.replay_buffer.full) == (host.replay_buffer.pos, host.replay_buffer.full)
    assert eng.n_target_syncs == host_syncs > 0
    assert algo.num_timesteps >= STEPS and algo._n_updates > 0
    assert algo.td_path == host.td_path == "fused"
    assert all(bool(th.isfinite(p).all()) for p in algo.q_net.parameters())
    assert any(not th.equal(a, b.detach()) for a, b in zip(p0, algo.q_net.parameters()))
    n = algo._td["layout"].n
    assert th.equal(algo._td["target"][:n], snap["online"][:n])
    assert not th.equal(algo._td["target"][:n], algo.policy.optimizer._flat[0]["flat"][:n])  # trained on since
    # the target modules read the bucket
    assert th.equal(next(algo.q_net_target.parameters()).detach().reshape(-1), algo._td["target"][: 64 * 4])


@pytest.mark.parametrize("kind", ["dqn", "sqil"])
def test_ring_holds_what_the_env_produced(kind, demos):
    n_envs = 4
    algo, eng, learn = _build(kind, n_envs, True, demos, env_id="CartPole-v1")
    rb = algo.replay_buffer
    expert0 = [t.clone() for t in rb.expert_buffer.td_fields()] if kind == "sqil" else None
    cb = _Mirror0(eng)
    learn(STEPS, callback=cb)
    T = algo.num_timesteps // n_envs
    assert T == rb.pos and not rb.full
    D = 4
    ring2 = [th.zeros(T * n_envs, D, device="cuda"), th.zeros(T * n_envs, D, device="cuda"),
             th.zeros(T * n_envs, 1, dtype=th.int64, device="cuda"), th.zeros(T * n_envs, device="cuda"),
             th.zeros(T * n_envs, device="cuda"), th.zeros(T * n_envs, device="cuda")]
    sq = kind == "sqil"
    rec = td.collect_records(T, n_envs, 2, "cuda")
    td.dqn_collect_reference(cb.env0, ring2, 0, T, algo.policy.optimizer._flat[0]["flat"], algo._td["layout"],
                             rb.actions[:T, :, 0], reward_const=0.0 if sq else None, write_timeouts=not sq, records=rec)
    got = rb.td_fields()
    for name, a, b in zip(("obs", "next_obs", "actions", "rewards", "dones", "timeouts"), got, ring2):
        assert th.equal(a[: T * n_envs], b), name
    assert int(ring2[4].sum()) > 0  # random CartPole episodes ended
    # the replayed envs stand where the engine's do
    for key in ("state", "rng", "elapsed", "ep_ret", "cur_obs"):
        assert th.equal(cb.env0[key], eng._env_tensors()[key]), key
    if sq:
        assert float(rb.rewards.abs().max()) == 0.0 and float(rb.timeouts.abs().max()) == 0.0
        for a, b in zip(expert0, rb.expert_buffer.td_fields()):
            assert th.equal(a, b)
        assert float(rb.expert_buffer.rewards.min()) == 1.0
    else:
        assert float(rb.rewards[:T].min()) == 1.0


def test_logging_and_host_continuation(demos, monkeypatch):
    n_envs = 4
    algo, eng, learn = _build("dqn", n_envs, True, demos, env_id="CartPole-v1")
    dumps = {"n": 0}
    real_dump = algo._dump_logs

    def dump():
        dumps["n"] += 1
        real_dump()

    monkeypatch.setattr(algo, "_dump_logs", dump)
    learn(STEPS, log_interval=4)
    rb = algo.replay_buffer
    T = algo.num_timesteps // n_envs
    dones = rb.dones[:T].cpu().numpy() > 0.5
    rews = rb.rewards[:T].cpu().numpy()
    want = []  # recount from the ring, in completion order: step, then env
    start = np.zeros(n_envs, dtype=np.int64)
    for t, n in zip(*(x.tolist() for x in np.nonzero(dones))):
        want.append((float(rews[start[n] : t + 1, n].sum()), int(t + 1 - start[n])))
        start[n] = t + 1
    got = [(ep["r"], ep["l"]) for ep in algo.ep_info_buffer]
    assert len(want) >= 8 and got == want
    assert all(set(ep) == {"r", "l", "t"} for ep in algo.ep_info_buffer)
    assert algo._episode_num == len(want) and dumps["n"] == len(want) // 4
    assert not eng._pending
    # the host venv continues from the device state
    nat = eng._native
    st = nat.get_state()
    assert np.array_equal(st["state"], eng.state.cpu().numpy())
    assert np.array_equal(st["rng"].astype(np.int64), eng.env_rng.cpu().numpy())
    assert np.array_equal(st["elapsed"].astype(np.int64), eng.elapsed.cpu().numpy().astype(np.int64))
    assert np.array_equal(algo._last_obs, eng.cur_obs.cpu().numpy())
    env = {k: (v.clone() if isinstance(v, th.Tensor) else v) for k, v in eng._env_tensors().items()}
    acts = th.tensor([[0, 1, 1, 0]], device="cuda")
    ring = [th.zeros(n_envs, 4, device="cuda"), th.zeros(n_envs, 4, device="cuda"),
            th.zeros(n_envs, 1, dtype=th.int64, device="cuda")] + [th.zeros(n_envs, device="cuda") for _ in range(3)]
    td.dqn_collect_reference(env, ring, 0, 1, algo.policy.optimizer._flat[0]["flat"], algo._td["layout"], acts,
                             records=td.collect_records(1, n_envs, 2, "cuda"))
    obs, rew, done, infos = algo.get_env().step(acts[0].cpu().numpy())
    nxt = np.stack([infos[i]["terminal_observation"] if done[i] else obs[i] for i in range(n_envs)])
    np.testing.assert_allclose(nxt, ring[1].cpu().numpy(), rtol=1e-5, atol=1e-6)
    assert np.array_equal(done, ring[4].cpu().numpy() > 0.5)


def test_train_imitation_sqil_routes_to_the_device_engine(tmp_path, monkeypatch, caplog):
    import logging

    from imitation_amd.scripts.train_imitation import train_imitation_ex

    monkeypatch.chdir(tmp_path)
    results = {}
    for engine in ("device", "host"):
        with caplog.at_level(logging.INFO, logger="imitation_amd.scripts.train_imitation"):
            caplog.clear()
            run = train_imitation_ex.run("sqil", named_configs=["fast", "demonstrations.fast", "environment.fast",
                                                                "policy_evaluation.fast"],
                                         config_updates={"logging": {"log_root": str(tmp_path / engine)},
                                                         "sqil": {"engine": engine}})
            assert f"sqil: {engine} engine" in caplog.text
        assert run.status == "COMPLETED" and run.config["sqil"]["engine"] == engine
        results[engine] = run.result
    assert set(results["device"]) == set(results["host"]) and "imit_stats" in results["device"]
    assert set(results["device"]["imit_stats"]) == set(results["host"]["imit_stats"])


def learning_run(seed, engine, demos):
    """The shape of the learning test in ``tests/rl/test_dqn_fused.py``: returns of 100 episodes
    before and after 1000 steps of DQN-SQIL on CartPole with 4 envs."""
    venv = _venv(4)
    model = sqil.SQIL(venv=venv, demonstrations=demos, policy="MlpPolicy", rl_algo_class=DQN, engine=engine,
                      rl_kwargs=dict(learning_starts=500, learning_rate=0.002, batch_size=220, seed=seed, device="cuda"))
    venv.seed(seed)
    before, _ = evaluation.evaluate_policy(model.policy, venv, 100, return_episode_rewards=True)
    model.train(total_timesteps=1_000)
    venv.seed(seed)
    after, _ = evaluation.evaluate_policy(model.policy, venv, 100, return_episode_rewards=True)
    return before, after, model.engine_kind


def test_sqil_learns_on_the_device_engine(cartpole_expert_trajectories):
    """Both the device engine and the host control improve the return significantly."""
    demos = rollout.flatten_trajectories(cartpole_expert_trajectories)
    for engine in ("device", "host"):
        before, after, kind = learning_run(LEARNING_SEED, engine, demos)
        assert kind == engine
        print(f"sqil learning seed {LEARNING_SEED} engine {kind}: before {np.mean(before):.1f} after {np.mean(after):.1f}")
        assert reward_improvement.is_significant_reward_improvement(before, after), (kind, np.mean(before), np.mean(after))
