"""Device-resident PPO on the environment reward -- the MI355X fast path of
``scripts/train_rl.py`` (reference ``src/imitation/scripts/train_rl.py``: SB3 ``PPO.learn`` on
a ``VecNormalize(norm_obs=False)`` venv).

=================================  ==================================================
reference                          this engine
=================================  ==================================================
``algo.learn(total_timesteps)``    device rounds of the generator core (:mod:`.generator`):
(collect_rollouts + PPO.train)     rollout chain kernel (policy + env physics), parallel
                                   value / log-prob / TimeLimit-bootstrap pass, GAE
                                   kernel, persistent PPO kernel
``VecNormalize(norm_obs=False)``   ONE ``reward_retnorm_kernel`` launch per round over the
(numpy, once per env step)         round's ``[T, N]`` env rewards and dones; the running
                                   return statistics and the envs' discounted returns
                                   stay on the device in fp64 (``ops.rl.return_normalize``)
callbacks (``on_step`` per env     driven once per round, after ``num_timesteps`` advanced
step)                              (``EveryNTimesteps`` fires at the same timestep counts
                                   whenever its period is a multiple of the round size)
=================================  ==================================================

The PPO object keeps its policy (parameters become views of the engine's flat buffer), so
saving, prediction and host-side evaluation after ``learn`` work on it unchanged.
"""

from __future__ import annotations

import collections
import math
import time
from typing import Any, Dict, Mapping, Optional, Tuple

import numpy as np
import torch as th

from imitation_amd.engine.generator import DeviceGeneratorCore, supports_generator
from imitation_amd.envs.vec_env import VecNormalize, is_vecenv_wrapped
from imitation_amd.ops import rl as rl_ops
from imitation_amd.parallel import dist as pdist
from imitation_amd.rl.callbacks import convert_callback


def supports(venv, algorithm) -> Tuple[bool, str]:
    """Whether :class:`DevicePPO` can train ``algorithm`` on ``venv`` (reason when not)."""
    ok, why = supports_generator(venv, algorithm)
    if not ok:
        return ok, why
    if pdist.world_size() > 1:
        return False, "data parallel (the return statistics would need a cross-rank merge)"
    if is_vecenv_wrapped(venv, VecNormalize):
        return False, "venv is wrapped in VecNormalize (pass normalize_reward to the engine instead)"
    return True, ""


class DevicePPO(DeviceGeneratorCore):
    """``algorithm.learn`` as device rounds on the env reward, with SB3 ``VecNormalize``
    reward normalisation on the GPU when ``normalize_reward`` (module docstring).
    ``normalize_kwargs``: ``gamma``, ``clip_reward`` and ``epsilon`` of ``VecNormalize``."""

    def __init__(self, algorithm, venv, normalize_reward: bool = False,
                 normalize_kwargs: Optional[Mapping[str, Any]] = None, custom_logger=None) -> None:
        ok, why = supports(venv, algorithm)
        if not ok:
            raise ValueError(f"DevicePPO not applicable: {why}; use PPO.learn")
        kw = dict(normalize_kwargs or {})
        self.norm_gamma = float(kw.pop("gamma", 0.99))
        self.norm_clip = float(kw.pop("clip_reward", 10.0))
        self.norm_eps = float(kw.pop("epsilon", 1e-8))
        kw.pop("norm_reward", None)
        if kw:
            raise ValueError(f"DevicePPO: unsupported normalize_kwargs {sorted(kw)}")
        self.gen_algo = algorithm
        self.venv = venv
        self._reward_net = None
        self.debug_use_ground_truth = True
        self.normalize_reward = bool(normalize_reward)
        if custom_logger is not None:
            algorithm.set_logger(custom_logger)
        self._init_generator(venv)
        # VecNormalize's state: the envs' discounted returns and RunningMeanStd() of them
        self.ret = th.zeros(self.N, dtype=th.float64, device=self._dev)
        self.rms = th.tensor([0.0, 1.0, 1e-4], dtype=th.float64, device=self._dev)
        self._ret_work = th.empty(self.T, self.N, dtype=th.float64, device=self._dev)
        self._ep_len = np.zeros(self.N, dtype=np.int64)

    # ------------------------------------------------------------------ the wrapped PPO's surface
    @property
    def logger(self):
        return self.gen_algo.logger

    @property
    def policy(self):
        return self.gen_algo.policy

    @property
    def num_timesteps(self) -> int:
        return self.gen_algo.num_timesteps

    def save(self, *args, **kwargs):
        return self.gen_algo.save(*args, **kwargs)

    def get_env(self):
        return self.gen_algo.get_env()

    def predict(self, *args, **kwargs):
        return self.gen_algo.predict(*args, **kwargs)

    # ------------------------------------------------------------------ one round
    def _rollout(self) -> None:
        """Chain -> parallel pass (``rewards = env_rew + boot``) -> with ``normalize_reward`` one
        launch that rewrites ``rewards`` as SB3 sees them: the VecNormalize'd env reward, then
        the TimeLimit bootstrap added to it."""
        self._launch_chain()
        self._launch_post(False)
        if self.normalize_reward:
            b = self.buf
            rl_ops.return_normalize(b["env_rew"], b["dones"], b["boot"], self.ret, self.rms, gamma=self.norm_gamma,
                                    eps=self.norm_eps, clip=self.norm_clip, out=b["rewards"], work=self._ret_work)

    def _track_episodes(self) -> None:
        """Monitor's ``info["episode"]`` of the staged round into ``ep_info_buffer`` (completion
        order: step, then env)."""
        dones = self._host_stage[0].numpy() > 0.5
        ep_ret = self._host_stage[1].numpy()
        self._host_staged = False
        T = dones.shape[0]
        last = np.full(self.N, -1, dtype=np.int64)
        buf = self.gen_algo.ep_info_buffer
        for t, n in zip(*(x.tolist() for x in np.nonzero(dones))):
            buf.append({"r": float(ep_ret[t, n]), "l": int(self._ep_len[n] + t - last[n]), "t": 0.0})
            self._ep_len[n] = 0
            last[n] = t
        self._ep_len += T - 1 - last

    def _log_round(self) -> None:
        self._record_round_metrics()
        self.logger.dump(step=self.gen_algo.num_timesteps)

    def learn(self, total_timesteps: int, callback=None, reset_num_timesteps: bool = True) -> "DevicePPO":
        """``PPO.learn``: rounds of ``n_steps * n_envs`` steps until ``num_timesteps`` reaches
        ``total_timesteps``. ``callback`` (anything ``PPO.learn`` accepts; its model is the
        wrapped PPO) sees ``on_rollout_start`` / ``on_rollout_end`` and ONE ``on_step`` per
        round; an ``on_step`` returning False stops the training after that round's update."""
        algo = self.gen_algo
        per_round = self.T * self.N
        if reset_num_timesteps or algo.ep_info_buffer is None:
            algo.ep_info_buffer = collections.deque(maxlen=algo._stats_window_size)
        if reset_num_timesteps:
            algo.num_timesteps = 0
        else:
            total_timesteps += algo.num_timesteps
        n_rounds = max(0, math.ceil((total_timesteps - algo.num_timesteps) / per_round))
        algo._total_timesteps = total_timesteps
        algo.start_time = time.time_ns()
        callback = convert_callback(callback)
        callback.init_callback(algo)
        callback.on_training_start(locals(), globals())
        self._fps_mark = (time.perf_counter(), algo.num_timesteps)
        logged = True
        for _ in range(n_rounds):
            callback.on_rollout_start()
            self._rollout()
            ready = self._stage_rollout_to_host()
            if not logged:
                # the previous round's records are written with this round's rollout already
                # queued behind its update (DeviceAgentTrainer.train): same values and steps
                self._log_round()
                logged = True
            algo.num_timesteps += per_round
            self._ppo_update()
            ready.synchronize()
            self._track_episodes()
            logged = False
            callback.on_rollout_end()
            if not callback.on_step():
                break
        if not logged:
            self._log_round()
        callback.on_training_end()
        self.check_errors(blocking=True)
        self.sync_env_to_host()  # (host-side rollouts / evaluation continue from the training env state)
        return self

    # ------------------------------------------------------------------ checkpoint
    _ENGINE_TENSORS = DeviceGeneratorCore._ENGINE_TENSORS + ("ret", "rms")

    def engine_state(self) -> Dict[str, Any]:
        """Everything a resumed trainer needs beyond the policy's ``state_dict``."""
        return dict(self._core_engine_state(), ep_len=th.as_tensor(self._ep_len.copy()),
                    num_timesteps=int(self.gen_algo.num_timesteps), n_updates=int(self.gen_algo._n_updates))

    def load_engine_state(self, st: Dict[str, Any]) -> None:
        self._load_core_engine_state(st)
        self._ep_len = st["ep_len"].numpy().copy()
        self.gen_algo.num_timesteps = int(st["num_timesteps"])
        self.gen_algo._n_updates = int(st["n_updates"])
        self.sync_env_to_host()
