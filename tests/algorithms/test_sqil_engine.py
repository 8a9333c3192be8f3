"""``SQIL(engine=...)``: the choice between the host loop and the device engine
(``engine/dqn.py``), and the host-side pieces of the device collection (``ops/dqn.py``)."""

import numpy as np
import pytest
import torch as th

from imitation_amd.algorithms import sqil
from imitation_amd.data import types
from imitation_amd.ops import dqn as td
from imitation_amd.rl.dqn import DQN


def _venv(env_id="seals/CartPole-v0", n_envs=1):
    from imitation_amd.util.util import make_vec_env

    return make_vec_env(env_id, rng=np.random.default_rng(0), n_envs=n_envs)


def _demos(venv, n=12):
    rng = np.random.default_rng(1)
    space = venv.observation_space
    if space.dtype == np.uint8:
        obs = rng.integers(0, 255, (n + 1, *space.shape), dtype=np.uint8)
    else:
        obs = rng.standard_normal((n + 1, *space.shape)).astype(np.float32)
    acts = rng.integers(0, venv.action_space.n, n)
    return types.Transitions(obs=obs[:-1], acts=acts, infos=np.array([{}] * n), next_obs=obs[1:],
                             dones=np.zeros(n, dtype=bool))


def _sqil(venv=None, policy="MlpPolicy", **kw):
    venv = venv or _venv()
    rl_kwargs = dict(learning_starts=20, batch_size=8, buffer_size=200, seed=0, device="cpu")
    rl_kwargs.update(kw.pop("rl_kwargs", {}))
    return sqil.SQIL(venv=venv, demonstrations=_demos(venv), policy=policy, rl_algo_class=DQN, rl_kwargs=rl_kwargs, **kw)


@pytest.fixture
def no_gpu(monkeypatch):
    monkeypatch.setattr(th.cuda, "is_available", lambda: False)


def test_host_is_the_default():
    model = _sqil()
    assert model.engine_kind == "host" and model._engine is None
    assert _sqil(engine="host").engine_kind == "host"


def test_device_without_a_gpu_names_the_reason(no_gpu):
    with pytest.raises(ValueError, match="no GPU"):
        _sqil(engine="device")


def test_device_rejects_a_cnn_policy(no_gpu):
    with pytest.raises(ValueError, match="image observations|not a vector-observation MLP"):
        _sqil(venv=_venv("PongNoFrameskip-v4"), policy="CnnPolicy", engine="device", rl_kwargs=dict(buffer_size=8))


@pytest.mark.parametrize("train_freq,reason", [((1, "episode"), "episodes, not steps"), (32, "32 steps")])
def test_device_rejects_train_freq(train_freq, reason, no_gpu):
    with pytest.raises(ValueError, match=reason):
        _sqil(engine="device", rl_kwargs=dict(train_freq=train_freq))


def test_auto_falls_back_and_trains(no_gpu):
    model = _sqil(engine="auto")
    assert model.engine_kind == "host"
    p0 = [p.detach().clone() for p in model.rl_algo.q_net.parameters()]
    model.train(total_timesteps=60)
    assert model.rl_algo.num_timesteps >= 60 and model.rl_algo._n_updates > 0
    assert any(not th.equal(a, b.detach()) for a, b in zip(p0, model.rl_algo.q_net.parameters()))


def test_unknown_engine_raises():
    with pytest.raises(ValueError, match="'host', 'device' or 'auto'"):
        _sqil(engine="gpu")


def test_explore_thresholds():
    assert td.explore_thresholds([0.0, 1.0, 0.05]) == [0, 1 << 24, 838860]  # 0.05 * 2^24 = 838860.8
    assert td.explore_thresholds([1e-9, 0.5, 1.0 - 1e-12, 1.5, -0.5]) == [0, 1 << 23, (1 << 24) - 1, 1 << 24, 0]
    eps = np.linspace(0.0, 1.0, 257)
    thr = td.explore_thresholds(eps)
    assert all(a <= b for a, b in zip(thr, thr[1:])) and len(set(thr)) == len(thr)


def test_splitmix_mirror_reproduces_the_native_env_reset():
    """CartPole's reset draws four 24-bit uniforms from ``seed_stream(seed, env)``: the mirror gives
    the env's stream state after the reset exactly, and the state the draws map to."""
    from imitation_amd.envs.vec_env import NativeVecEnv

    for seed in (0, 3, 2**40 + 17):
        venv = NativeVecEnv("CartPole-v1", 1, seed=seed)
        obs = venv.reset()
        s = td.seed_stream(seed, 0)
        draws = []
        for _ in range(4):
            s, u = td.draw24(s)
            draws.append(u)
        assert td.stream_states(th.as_tensor(venv.get_state()["rng"])) == [s]
        want = np.float32(-0.05) + np.float32(0.1) * (np.asarray(draws, np.float32) * np.float32(2.0**-24))
        np.testing.assert_allclose(obs[0], want, rtol=0, atol=1e-8)
        assert all(0 <= u < (1 << 24) for u in draws)
