"""``DQN`` / ``SQIL`` on the fused one-launch TD step (``rl/dqn.py``; ``ops/dqn.py``)."""

import numpy as np
import pytest
import torch as th

from imitation_amd.algorithms import sqil
from imitation_amd.data import rollout
from imitation_amd.ops import dqn as td
from imitation_amd.ops.optim import FusedAdam
from imitation_amd.rl import dqn as dqn_mod
from imitation_amd.rl import evaluation
from imitation_amd.rl.dqn import DQN
from imitation_amd.testing import reward_improvement

pytestmark = pytest.mark.gpu

# seed of the learning test: the first of 42, 43, ... at which the eager control passes on the card
LEARNING_SEED = 42


def _venv(n_envs=1):
    from imitation_amd.data.wrappers import RolloutInfoWrapper
    from imitation_amd.util.util import make_vec_env

    return make_vec_env("seals/CartPole-v0", rng=np.random.default_rng(0), n_envs=n_envs,
                        post_wrappers=[lambda e, _: RolloutInfoWrapper(e)])


@pytest.fixture
def demos(cartpole_expert_trajectories):
    return rollout.flatten_trajectories(cartpole_expert_trajectories[:8])


def _build(kind, demos, n_envs=1, **kw):
    kwargs = dict(learning_starts=50, batch_size=32, seed=0, device="cuda")
    kwargs.update(kw)
    if kind == "dqn":
        algo = DQN("MlpPolicy", _venv(n_envs), **kwargs)
        return algo, algo, lambda steps: algo.learn(steps)
    model = sqil.SQIL(venv=_venv(n_envs), demonstrations=demos, policy="MlpPolicy", rl_algo_class=DQN, rl_kwargs=kwargs)
    return model, model.rl_algo, lambda steps: model.train(total_timesteps=steps)


@pytest.mark.parametrize("kind,n_envs", [("dqn", 1), ("sqil", 1), ("sqil", 4)])
def test_fused_run_trains_saves_and_loads(kind, n_envs, demos, tmp_path):
    _, algo, learn = _build(kind, demos, n_envs)
    p0 = [p.detach().clone() for p in algo.q_net.parameters()]
    learn(200)
    assert algo.td_path == "fused"
    assert algo._n_updates > 0
    assert any(not th.equal(a, b.detach()) for a, b in zip(p0, algo.q_net.parameters()))
    assert all(bool(th.isfinite(p).all()) for p in algo.q_net.parameters())
    opt = algo.policy.optimizer
    assert isinstance(opt, FusedAdam)
    assert float(opt.step_counter()) == algo._n_updates
    # .grad is populated, as the eager path leaves it
    assert all(p.grad is not None for p in algo.q_net.parameters())
    assert any(float(p.grad.abs().max()) > 0 for p in algo.q_net.parameters())
    # the optimizer state interchanges with torch's Adam
    clones = [th.nn.Parameter(p.detach().clone()) for p in algo.q_net.parameters()]
    adam = th.optim.Adam(clones, lr=1e-4)
    adam.load_state_dict(opt.state_dict())
    for c, p in zip(clones, algo.q_net.parameters()):
        th.testing.assert_close(adam.state[c]["exp_avg"], opt.state[p]["exp_avg"])
        assert float(adam.state[c]["step"]) == algo._n_updates
    # save, load on the CPU: the Q-values of a fixed observation batch
    obs = th.randn(16, 4, generator=th.Generator().manual_seed(0))
    with th.no_grad():
        q_gpu = algo.q_net(obs.cuda()).cpu()
    path = str(tmp_path / "model.zip")
    algo.save(path)
    loaded = DQN.load(path, device="cpu")
    assert loaded.td_path is None and loaded._td is None
    with th.no_grad():
        th.testing.assert_close(loaded.q_net(obs), q_gpu)
        th.testing.assert_close(loaded.q_net_target(obs), algo.q_net_target(obs.cuda()).cpu())


@pytest.mark.parametrize("kind", ["dqn", "sqil"])
def test_knob_keeps_the_eager_step(kind, demos, monkeypatch):
    monkeypatch.setenv("IMITATION_AMD_DQN_FUSED", "0")
    _, algo, learn = _build(kind, demos)
    learn(80)
    assert algo.td_path == "eager:knob"
    assert algo._n_updates > 0 and not isinstance(algo.policy.optimizer, FusedAdam)


def _first_train_call(kind, demos, fused, monkeypatch):
    """Run until the first ``train()`` call returns: the ``th.randint`` results drawn inside it, its
    loss, and (fused) the fp64 / fp32-eager evaluations of the step from the state before it."""
    rec = {"ids": [], "inside": False}
    with monkeypatch.context() as mp:
        mp.setenv("IMITATION_AMD_DQN_FUSED", "1" if fused else "0")
        _, algo, learn = _build(kind, demos)
        real_randint, real_train, real_step, real_l1 = th.randint, algo.train, td.dqn_td_step, dqn_mod.F.smooth_l1_loss

        class Done(Exception):
            pass

        def randint(*a, **k):
            out = real_randint(*a, **k)
            if rec["inside"]:
                rec["ids"].append(out.clone())
            return out

        def train(*a, **k):
            rec["inside"] = True
            real_train(*a, **k)
            raise Done

        def step(src_a, src_b, ids_a, ids_b, flat, grad, m, v, stp, target, layout, **k):
            for name, dtype in (("loss64", th.float64), ("loss32", th.float32)):
                st = [t.clone().to(dtype) for t in (flat, grad, m, v, stp, target)]
                cast = lambda s: None if s is None else [t if t.dtype == th.int64 else t.to(dtype) for t in s]  # noqa: E731
                rec[name] = td.dqn_td_reference(cast(src_a), cast(src_b), ids_a, ids_b, *st, layout, **k)[0].clone()
            out = real_step(src_a, src_b, ids_a, ids_b, flat, grad, m, v, stp, target, layout, **k)
            rec["loss"] = out[0].clone()
            return out

        def l1(*a, **k):
            out = real_l1(*a, **k)
            rec["loss"] = out.detach().reshape(1).clone()
            return out

        mp.setattr(th, "randint", randint)
        mp.setattr(algo, "train", train)
        mp.setattr(td, "dqn_td_step", step)
        mp.setattr(dqn_mod.F, "smooth_l1_loss", l1)
        with pytest.raises(Done):
            learn(200)
    rec["td_path"] = algo.td_path
    return rec


@pytest.mark.parametrize("kind", ["dqn", "sqil"])
def test_fused_and_eager_draw_the_same_batches(kind, demos, monkeypatch):
    """From one seed the two paths draw bitwise equal row ids in the first ``train()`` call (agent
    step ids, agent env ids, expert step ids, expert env ids), and their first losses agree: the
    fused one within the bound of the kernel test (|fused - fp64| <= 4 |fp32 torch eager - fp64| +
    one fp32 ulp, both evaluations of that step from the state before it), the eager run's at
    torch's fp32 defaults against the same fp64 value."""
    fused = _first_train_call(kind, demos, True, monkeypatch)
    eager = _first_train_call(kind, demos, False, monkeypatch)
    assert fused["td_path"] == "fused" and eager["td_path"] == "eager:knob"
    assert len(fused["ids"]) == len(eager["ids"]) == (2 if kind == "dqn" else 4)
    for a, b in zip(fused["ids"], eager["ids"]):
        assert a.device.type == "cuda" and th.equal(a, b)
    l64 = float(fused["loss64"][0])
    err_f, err_32 = abs(float(fused["loss"][0]) - l64), abs(float(fused["loss32"][0]) - l64)
    print(f"first-step loss {kind}: fp64 {l64:.9g} fused err {err_f:.3e} fp32 reference err {err_32:.3e} "
          f"eager run err {abs(float(eager['loss'][0]) - l64):.3e}")
    assert err_f <= 4 * err_32 + float(np.spacing(np.float32(abs(l64))))
    # the eager run computed its loss on the same batch from the same state
    th.testing.assert_close(eager["loss"][0].cpu(), fused["loss64"][0].float().cpu())


def learning_run(seed, fused, demos, monkeypatch):
    """The shape of ``test_sqil_performance_discrete``: returns of 100 episodes before and after
    1000 steps of DQN-SQIL on CartPole."""
    with monkeypatch.context() as mp:
        mp.setenv("IMITATION_AMD_DQN_FUSED", "1" if fused else "0")
        venv = _venv(4)
        model = sqil.SQIL(venv=venv, demonstrations=demos, policy="MlpPolicy", rl_algo_class=DQN,
                          rl_kwargs=dict(learning_starts=500, learning_rate=0.002, batch_size=220, seed=seed,
                                         device="cuda"))
        venv.seed(seed)
        before, _ = evaluation.evaluate_policy(model.policy, venv, 100, return_episode_rewards=True)
        model.train(total_timesteps=1_000)
        venv.seed(seed)
        after, _ = evaluation.evaluate_policy(model.policy, venv, 100, return_episode_rewards=True)
    return before, after, model.rl_algo.td_path


def test_sqil_learns_fused_and_eager(cartpole_expert_trajectories, monkeypatch):
    """Both the fused run and the eager control (knob off) improve the return significantly."""
    demos = rollout.flatten_trajectories(cartpole_expert_trajectories)
    for fused in (True, False):
        before, after, path = learning_run(LEARNING_SEED, fused, demos, monkeypatch)
        assert path == ("fused" if fused else "eager:knob")
        print(f"sqil learning seed {LEARNING_SEED} {path}: before {np.mean(before):.1f} after {np.mean(after):.1f}")
        assert reward_improvement.is_significant_reward_improvement(before, after), (path, np.mean(before), np.mean(after))
