"""``SAC`` / ``SQIL`` with a SAC learner on the fused one-launch update (``rl/sac.py``; ``ops/sac.py``)."""

import numpy as np
import pytest
import torch as th

from imitation_amd.algorithms import sqil
from imitation_amd.data import rollout
from imitation_amd.ops.optim import FusedAdam
from imitation_amd.rl import logger as rl_logger
from imitation_amd.rl.sac import SAC

pytestmark = pytest.mark.gpu

LOSSES = ("train/critic_loss", "train/actor_loss", "train/ent_coef_loss")


def _venv(n_envs=1):
    from imitation_amd.data.wrappers import RolloutInfoWrapper
    from imitation_amd.util.util import make_vec_env

    return make_vec_env("Pendulum-v1", rng=np.random.default_rng(0), n_envs=n_envs,
                        post_wrappers=[lambda e, _: RolloutInfoWrapper(e)])


@pytest.fixture
def demos(pendulum_expert_trajectories):
    return rollout.flatten_trajectories(pendulum_expert_trajectories[:4])


def _build(kind, demos, **kw):
    kwargs = dict(learning_starts=50, batch_size=64, seed=0, device="cuda", policy_kwargs=dict(net_arch=[64, 64]))
    kwargs.update(kw)
    if kind == "sac":
        algo = SAC("MlpPolicy", _venv(), **kwargs)
        algo.set_logger(rl_logger.configure(None, []))  # (a logger that learn() keeps: the tests read what train() records)
        return algo, algo, lambda steps: algo.learn(steps)
    model = sqil.SQIL(venv=_venv(), demonstrations=demos, policy="MlpPolicy", rl_algo_class=SAC, rl_kwargs=kwargs)
    model.rl_algo.set_logger(rl_logger.configure(None, []))
    return model, model.rl_algo, lambda steps: model.train(total_timesteps=steps)


def _snapshot(algo):
    return dict(actor=[p.detach().clone() for p in algo.actor.parameters()],
                critic=[p.detach().clone() for p in algo.critic.parameters()],
                target=[p.detach().clone() for p in algo.critic_target.parameters()],
                log_ent_coef=[algo.log_ent_coef.detach().clone()])


def _moved(before, after):
    return {k: any(not th.equal(a, b) for a, b in zip(before[k], after[k])) for k in before}


@pytest.mark.parametrize("kind", ["sac", "sqil"])
def test_fused_run_trains_saves_and_loads(kind, demos, tmp_path):
    _, algo, learn = _build(kind, demos)
    seen = []
    real_record = algo.logger.record

    def record(key, value, *a, **k):
        if key in LOSSES:
            seen.append(float(value))
        return real_record(key, value, *a, **k)

    algo.logger.record = record
    before = _snapshot(algo)
    learn(300)
    assert algo.update_path == "fused"
    assert algo._n_updates >= 200
    assert _moved(before, _snapshot(algo)) == dict(actor=True, critic=True, target=True, log_ent_coef=True)
    assert len(seen) == 3 * algo._n_updates and all(np.isfinite(seen))  # (one gradient step per train() call)
    for p in list(algo.actor.parameters()) + list(algo.critic.parameters()) + list(algo.critic_target.parameters()):
        assert bool(th.isfinite(p).all())
    for opt in (algo.actor.optimizer, algo.critic.optimizer, algo.ent_coef_optimizer):
        assert isinstance(opt, FusedAdam)
        assert float(opt.step_counter()) == algo._n_updates
    # .grad is populated, as the eager path leaves it
    assert all(p.grad is not None for p in algo.actor.parameters())
    assert any(float(p.grad.abs().max()) > 0 for p in algo.actor.parameters())
    # the optimizer state interchanges with torch's Adam
    clones = [th.nn.Parameter(p.detach().clone()) for p in algo.critic.parameters()]
    adam = th.optim.Adam(clones, lr=3e-4)
    adam.load_state_dict(algo.critic.optimizer.state_dict())
    for c, p in zip(clones, algo.critic.parameters()):
        th.testing.assert_close(adam.state[c]["exp_avg"], algo.critic.optimizer.state[p]["exp_avg"])
        assert float(adam.state[c]["step"]) == algo._n_updates
    # save, load on the CPU: the actor and both critics on a fixed batch
    gen = th.Generator().manual_seed(0)
    obs, act = th.randn(16, 3, generator=gen), th.rand(16, 1, generator=gen) * 2 - 1
    with th.no_grad():
        a_gpu = algo.actor(obs.cuda(), deterministic=True).cpu()
        q_gpu = [q.cpu() for q in algo.critic(obs.cuda(), act.cuda())]
        t_gpu = [q.cpu() for q in algo.critic_target(obs.cuda(), act.cuda())]
    path = str(tmp_path / "model.zip")
    algo.save(path)
    loaded = SAC.load(path, device="cpu")
    assert loaded.update_path is None and loaded._sac is None
    with th.no_grad():
        th.testing.assert_close(loaded.actor(obs, deterministic=True), a_gpu)
        for q, ref in zip(loaded.critic(obs, act), q_gpu):
            th.testing.assert_close(q, ref)
        for q, ref in zip(loaded.critic_target(obs, act), t_gpu):
            th.testing.assert_close(q, ref)
    # load on the GPU and go on: the fused path again, from the loaded weights
    again = SAC.load(path, env=_venv(), device="cuda")
    mid = _snapshot(again)
    for a, b in zip(mid["critic"], algo.critic.parameters()):
        assert th.equal(a, b.detach())
    again.learn(100)
    assert again.update_path == "fused" and again._n_updates > algo._n_updates
    assert _moved(mid, _snapshot(again)) == dict(actor=True, critic=True, target=True, log_ent_coef=True)
    # the first model goes on as well
    n0 = algo._n_updates
    learn(60)
    assert algo.update_path == "fused" and algo._n_updates > n0


@pytest.mark.parametrize("kind", ["sac", "sqil"])
def test_knob_keeps_the_eager_step(kind, demos, monkeypatch):
    monkeypatch.setenv("IMITATION_AMD_SAC_FUSED", "0")
    _, algo, learn = _build(kind, demos)
    before = _snapshot(algo)
    learn(70)
    assert algo.update_path == "eager:knob"
    assert algo._n_updates > 0 and not isinstance(algo.actor.optimizer, FusedAdam)
    assert _moved(before, _snapshot(algo)) == dict(actor=True, critic=True, target=True, log_ent_coef=True)


def _first_train_call(kind, demos, fused, monkeypatch):
    """Run until the first ``train()`` call returns: the ``th.randint`` results and the normal
    noise drawn inside it, and the losses it logged."""
    rec = {"ids": [], "noise": [], "logged": {}, "inside": False}
    with monkeypatch.context() as mp:
        mp.setenv("IMITATION_AMD_SAC_FUSED", "1" if fused else "0")
        _, algo, learn = _build(kind, demos)
        real_randint, real_randn, real_randn_like, real_train = th.randint, th.randn, th.randn_like, algo.train
        logger = algo.logger
        real_record = logger.record

        class Done(Exception):
            pass

        def keep(name, real):
            def draw(*a, **k):
                out = real(*a, **k)
                if rec["inside"]:
                    rec[name].append(out.clone())
                return out

            return draw

        def record(key, value, *a, **k):
            if rec["inside"]:
                rec["logged"][key] = float(value)
            return real_record(key, value, *a, **k)

        def train(*a, **k):
            rec["inside"] = True
            real_train(*a, **k)
            raise Done

        mp.setattr(th, "randint", keep("ids", real_randint))
        mp.setattr(th, "randn", keep("noise", real_randn))
        mp.setattr(th, "randn_like", keep("noise", real_randn_like))
        mp.setattr(logger, "record", record)
        mp.setattr(algo, "train", train)
        with pytest.raises(Done):
            learn(200)
    rec["update_path"] = algo.update_path
    return rec


@pytest.mark.parametrize("kind", ["sac", "sqil"])
def test_fused_and_eager_draw_the_same_batches_and_noise(kind, demos, monkeypatch):
    """From one seed the two paths draw bitwise equal row ids (agent step ids, agent env ids, then
    the expert ring's) and bitwise equal actor noise (on the observations, then on the next
    observations) in the first ``train()`` call, and the three losses that call logs agree at
    torch's fp32 ``assert_close`` defaults."""
    fused = _first_train_call(kind, demos, True, monkeypatch)
    eager = _first_train_call(kind, demos, False, monkeypatch)
    assert fused["update_path"] == "fused" and eager["update_path"] == "eager:knob"
    assert len(fused["ids"]) == len(eager["ids"]) == (2 if kind == "sac" else 4)
    for a, b in zip(fused["ids"], eager["ids"]):
        assert a.device.type == "cuda" and th.equal(a, b)
    assert len(fused["noise"]) == len(eager["noise"]) == 2
    for a, b in zip(fused["noise"], eager["noise"]):
        assert a.device.type == "cuda" and a.shape == (64, 1) and th.equal(a, b)
    for key in LOSSES:
        print(f"first train() {kind} {key}: fused {fused['logged'][key]:.9g} eager {eager['logged'][key]:.9g}")
    for key in LOSSES + ("train/ent_coef",):
        th.testing.assert_close(th.tensor(fused["logged"][key], dtype=th.float32),
                                th.tensor(eager["logged"][key], dtype=th.float32))
