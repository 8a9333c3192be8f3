"""``engine_state`` / ``load_engine_state`` of the three device engines (CPU).

The real unbound methods of :class:`DeviceEngineMixin` (GAIL / AIRL), :class:`DevicePPO`
(``train_rl``) and :class:`DeviceAgentTrainer` (DRLHP) run on stand-ins that hold CPU tensors
in place of the device state. The key sets are the checkpoint format: they are spelled out
here, not derived from the code under test."""

import collections
import types

import numpy as np
import pytest
import torch as th

from imitation_amd.engine.gail import DeviceEngineMixin
from imitation_amd.engine.generator import DeviceGeneratorCore
from imitation_amd.engine.preference import DeviceAgentTrainer
from imitation_amd.engine.rl import DevicePPO

N, D, P = 3, 4, 10  # envs, obs dim, flat parameters
NINE = {"exp_avg", "exp_avg_sq", "adam_step", "state", "env_rng", "elapsed", "ep_ret", "cur_obs", "cur_start"}
COMMON = NINE | {"step0", "seed", "perm_round"}
OWN = {
    DeviceEngineMixin: {"ep_lens_running", "gen_dev", "gen_dev_idx", "gen_dev_n"},
    DevicePPO: {"ret", "rms", "ep_len", "num_timesteps", "n_updates"},
    DeviceAgentTrainer: {"explore_random"},
}
ENGINES = sorted(OWN, key=lambda c: c.__name__)


def _stand_in(cls, salt: int, norm: bool = True, wrapped: bool = False):
    """An object with the attributes ``cls``'s engine-state methods touch, filled from ``salt``."""

    class Engine:
        _ENGINE_TENSORS = cls._ENGINE_TENSORS
        _core_engine_state = DeviceGeneratorCore._core_engine_state
        _load_core_engine_state = DeviceGeneratorCore._load_core_engine_state
        engine_state = cls.engine_state
        load_engine_state = cls.load_engine_state

        def sync_env_to_host(self):
            self.synced += 1

        def _reset_accumulator(self):
            self.accumulator_resets += 1

    g = th.Generator().manual_seed(salt)
    e = Engine()
    e._dev = "cpu"
    e.synced = e.accumulator_resets = 0
    shapes = dict(exp_avg=(P,), exp_avg_sq=(P,), adam_step=(1,), state=(N, 6), ep_ret=(N,), cur_obs=(N, D),
                  cur_start=(N,))
    for k, s in shapes.items():
        setattr(e, k, th.rand(*s, generator=g))
    e.env_rng = th.randint(0, 2**62, (N, 2), generator=g)
    e.elapsed = th.randint(0, 1000, (N,), generator=g, dtype=th.int32)
    e.pol_norm = types.SimpleNamespace(count=th.tensor(100 + salt, dtype=th.int32)) if norm else None
    e.norm_count = th.tensor([float(100 + salt)]) if norm else None
    e._step0, e._seed, e._perm_round = 64 * salt, 12345 + salt, 7 + salt
    if cls is DeviceEngineMixin:
        e._ep_lens_running = np.arange(N, dtype=np.int64) + salt
        arrays = {"obs": th.rand(8, D, generator=g), "acts": th.randint(0, 2, (8,), generator=g),
                  "next_obs": th.rand(8, D, generator=g), "dones": th.rand(8, generator=g) < 0.5}
        e._gen_dev = types.SimpleNamespace(_arrays=arrays, _idx=salt % 8, _n_data=8 - salt % 3)
        if wrapped:
            e._wrapped_eps = collections.deque([1.5 * salt, -2.0], maxlen=100)
            e._wrapped_cum = np.linspace(0.0, 1.0, N) * salt
    elif cls is DevicePPO:
        e.ret = th.rand(N, generator=g, dtype=th.float64)
        e.rms = th.rand(3, generator=g, dtype=th.float64)
        e._ep_len = np.arange(N, dtype=np.int64) * salt
        e.gen_algo = types.SimpleNamespace(num_timesteps=4096 * salt, _n_updates=10 * salt)
    else:
        e._explore_random = bool(salt % 2)
    return e


def _assert_same(a, b, path=""):
    assert type(a) is type(b), (path, type(a), type(b))
    if isinstance(a, dict):
        assert set(a) == set(b), path
        for k in a:
            _assert_same(a[k], b[k], f"{path}/{k}")
    elif isinstance(a, th.Tensor):
        assert a.dtype == b.dtype and th.equal(a, b), path
    else:
        assert a == b, path


@pytest.mark.parametrize("cls", ENGINES, ids=lambda c: c.__name__)
@pytest.mark.parametrize("norm", [True, False], ids=["norm", "no_norm"])
def test_engine_state_key_set(cls, norm):
    want = COMMON | OWN[cls] | ({"norm_count"} if norm else set())
    assert set(_stand_in(cls, 1, norm=norm).engine_state()) == want
    if cls is DeviceEngineMixin:  # the wrapped-return bookkeeping appears once it has run
        st = _stand_in(cls, 1, norm=norm, wrapped=True).engine_state()
        assert set(st) == want | {"wrapped_eps", "wrapped_cum"}


@pytest.mark.parametrize("cls", ENGINES, ids=lambda c: c.__name__)
def test_engine_state_round_trip(cls):
    src = _stand_in(cls, 1, wrapped=True)
    st = src.engine_state()
    dst = _stand_in(cls, 2)
    tensors = {k: getattr(dst, k) for k in cls._ENGINE_TENSORS}
    dst.load_engine_state(st)
    assert th.equal(dst.norm_count, st["norm_count"])
    # a resume loads the policy's state_dict as well, and a save re-reads the module's count
    dst.pol_norm.count.copy_(src.pol_norm.count)
    _assert_same(dst.engine_state(), st)
    assert all(getattr(dst, k) is t for k, t in tensors.items())  # loaded in place
    assert (dst._step0, dst._seed, dst._perm_round) == (src._step0, src._seed, src._perm_round)
    assert dst.synced == 1
    if cls is DeviceEngineMixin:
        assert np.array_equal(dst._ep_lens_running, src._ep_lens_running)
        assert list(dst._wrapped_eps) == list(src._wrapped_eps) and dst._wrapped_eps.maxlen == 100
        assert np.array_equal(dst._wrapped_cum, src._wrapped_cum)
        assert (dst._gen_dev._idx, dst._gen_dev._n_data) == (src._gen_dev._idx, src._gen_dev._n_data)
    elif cls is DevicePPO:
        assert np.array_equal(dst._ep_len, src._ep_len)
        assert vars(dst.gen_algo) == vars(src.gen_algo)
    else:
        assert dst._explore_random is src._explore_random
        assert dst.accumulator_resets == 1


@pytest.mark.parametrize("cls", ENGINES, ids=lambda c: c.__name__)
def test_state_without_perm_round_loads_as_zero(cls):
    st = _stand_in(cls, 1).engine_state()
    del st["perm_round"]
    dst = _stand_in(cls, 2)
    dst.load_engine_state(st)
    assert dst._perm_round == 0


@pytest.mark.parametrize("cls", ENGINES, ids=lambda c: c.__name__)
def test_saved_norm_count_is_the_modules(cls):
    e = _stand_in(cls, 1)
    e.pol_norm.count.fill_(4321)  # (the single-rank update advances the module's count only)
    st = e.engine_state()
    assert st["norm_count"].dtype == th.float32 and st["norm_count"].tolist() == [4321.0]
