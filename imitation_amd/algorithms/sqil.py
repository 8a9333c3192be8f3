"""Soft Q Imitation Learning (reference: ``src/imitation/algorithms/sqil.py``).

Off-policy RL (DQN by default; SAC/TD3-style learners also accepted) on a replay
buffer that serves 50 % expert transitions with reward 1 and 50 % agent
transitions with reward 0 (``sqil.py:196-251``). Both halves live in device
replay rings; the expert half is bulk-uploaded once.
"""

from __future__ import annotations

import logging
from typing import Any, Dict, List, Optional, Type, Union

import numpy as np
import torch as th

from imitation_amd.algorithms import base as algo_base
from imitation_amd.data import rollout, types
from imitation_amd.envs import spaces
from imitation_amd.rl import buffers
from imitation_amd.rl.dqn import DQN
from imitation_amd.util import logger, util


class SQIL(algo_base.DemonstrationAlgorithm[types.Transitions]):
    """Soft Q Imitation Learning (SQIL), Reddy et al. 2019."""

    def __init__(self, *, venv, demonstrations: Optional[algo_base.AnyTransitions], policy,
                 custom_logger: Optional[logger.HierarchicalLogger] = None, rl_algo_class=DQN,
                 rl_kwargs: Optional[Dict[str, Any]] = None, engine: str = "host"):
        """``engine``: ``"host"`` trains with the learner's own ``learn`` loop; ``"device"`` with
        :class:`imitation_amd.engine.dqn.DeviceDQN` (acting, env stepping and replay writes on the
        GPU; ``ValueError`` with the reason when the run is not eligible); ``"auto"`` uses the
        device engine when eligible and the host loop otherwise."""
        if engine not in ("host", "device", "auto"):
            raise ValueError(f"SQIL engine must be 'host', 'device' or 'auto', not {engine!r}")
        self.venv = venv
        if rl_kwargs is None:
            rl_kwargs = {}
        if "replay_buffer_class" in rl_kwargs:
            raise ValueError("SQIL uses a custom replay buffer: 'replay_buffer_class' not allowed.")
        if "replay_buffer_kwargs" in rl_kwargs:
            raise ValueError("SQIL uses a custom replay buffer: 'replay_buffer_kwargs' not allowed.")
        self.rl_algo = rl_algo_class(policy=policy, env=venv, replay_buffer_class=SQILReplayBuffer,
                                     replay_buffer_kwargs={"demonstrations": demonstrations}, **rl_kwargs)
        super().__init__(demonstrations=demonstrations, custom_logger=custom_logger)
        self._engine = None
        if engine != "host":
            from imitation_amd.engine import dqn as dqn_engine

            ok, why = dqn_engine.supports(venv, self.rl_algo)
            if ok:
                self._engine = dqn_engine.DeviceDQN(self.rl_algo, venv)
            elif engine == "device":
                raise ValueError(f"SQIL engine='device' is not applicable: {why}")
            else:
                logging.getLogger(__name__).info("SQIL: host loop (device engine not applicable: %s)", why)

    @property
    def engine_kind(self) -> str:
        """``"device"`` when :meth:`train` runs the device engine, else ``"host"``."""
        return "host" if self._engine is None else "device"

    def set_demonstrations(self, demonstrations: algo_base.AnyTransitions) -> None:
        assert isinstance(self.rl_algo.replay_buffer, SQILReplayBuffer)
        self.rl_algo.replay_buffer.set_demonstrations(demonstrations)

    def train(self, *, total_timesteps: int, tb_log_name: str = "SQIL", **kwargs: Any):
        learner = self.rl_algo if self._engine is None else self._engine
        learner.learn(total_timesteps=total_timesteps, tb_log_name=tb_log_name, **kwargs)

    @property
    def policy(self):
        return self.rl_algo.policy


class SQILReplayBuffer(buffers.ReplayBuffer):
    """Replay buffer mixing agent (reward 0) and expert (reward 1) transitions half/half."""

    def __init__(self, buffer_size: int, observation_space: spaces.Space, action_space: spaces.Space,
                 demonstrations: algo_base.AnyTransitions, device: Union[th.device, str] = "auto", n_envs: int = 1,
                 optimize_memory_usage: bool = False):
        super().__init__(buffer_size=buffer_size, observation_space=observation_space, action_space=action_space,
                         device=device, n_envs=n_envs, optimize_memory_usage=optimize_memory_usage,
                         handle_timeout_termination=False)
        self.expert_buffer = buffers.ReplayBuffer(buffer_size=0, observation_space=observation_space,
                                                  action_space=action_space, device=device)
        self.set_demonstrations(demonstrations)

    def set_demonstrations(self, demonstrations: algo_base.AnyTransitions) -> None:
        if not isinstance(demonstrations, types.Transitions):
            item, demonstrations = util.get_first_iter_element(demonstrations)  # type: ignore[assignment]
            if isinstance(item, types.Trajectory):
                demonstrations = rollout.flatten_trajectories(demonstrations)  # type: ignore[arg-type]
        if not isinstance(demonstrations, types.Transitions):
            raise NotImplementedError(f"Unsupported demonstrations type: {demonstrations}")
        n = len(demonstrations)
        self.expert_buffer = buffers.ReplayBuffer(buffer_size=n, observation_space=self.observation_space,
                                                  action_space=self.action_space, device=self.device,
                                                  handle_timeout_termination=False)
        self.expert_buffer.extend(np.asarray(demonstrations.obs), np.asarray(demonstrations.next_obs),
                                  np.asarray(demonstrations.acts), np.ones(n, dtype=np.float32),
                                  np.asarray(demonstrations.dones, dtype=np.float32))

    def add(self, obs, next_obs, action, reward, done, infos: List[Dict[str, Any]]) -> None:
        super().add(obs=obs, next_obs=next_obs, action=action, reward=np.array(0.0), done=done, infos=infos)

    def td_sources(self, batch_size: int) -> List[Any]:
        """The agent ring and the expert ring with ``sample``'s half/half row counts."""
        new_size, expert_size = util.split_in_half(batch_size)
        return [(self, new_size), (self.expert_buffer, expert_size)]

    def sample(self, batch_size: int, env=None) -> buffers.ReplayBufferSamples:
        new_size, expert_size = util.split_in_half(batch_size)
        new_sample = super().sample(new_size, env)
        expert_sample = self.expert_buffer.sample(expert_size, env)
        return buffers.ReplayBufferSamples(*(th.cat((getattr(new_sample, n), getattr(expert_sample, n))) for n in new_sample._fields))
