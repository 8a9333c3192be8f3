"""Device-resident DQN / SQIL training: acting, env stepping and replay-ring writes of a
``train_freq`` chunk in ONE launch, then the fused TD launch -- no host wait per iteration.

=====================================  ==================================================
host loop (``rl/off_policy.py``)       this engine
=====================================  ==================================================
``collect_rollouts``: per env step a   ONE ``dqn_collect`` launch per ``train_freq`` steps
Q forward + ``.cpu()`` for the         (``csrc/kernels/dqn_collect.hip``, one wave per env):
action, ``NativeVecEnv.step``,         Q forward from the online flat bucket, greedy action,
``ReplayBuffer.add`` (six copies)      exploration coin, env physics with TimeLimit and
                                       auto-reset, the ring row (SQIL: reward 0, no timeouts)
``np.random.rand() < eps`` once per    a coin PER ENV from the env's device action stream
step for the whole batch, random       (``splitmix64``, integer-exact against
actions from ``action_space.sample``   ``floor(eps * 2^24)``); identical in distribution at
                                       ``n_envs = 1``; actions never come from ``np.random``
``_on_step`` per env step              applied on the host for the whole chunk without a
(``_n_calls``, target sync,            device read, at the timestep counts the host loop
``exploration_rate``)                  uses: the rate set after step ``i - 1`` decides step
                                       ``i``; target syncs that fall into the chunk run after
                                       its launch (the online weights do not change inside it)
``train()``: fused TD launch, then     the same launch (``DQN._td_launch``: the same
``float(losses.mean())``               ``th.randint`` calls in the same order); the loss stays
                                       on the device and reaches the logger with the records
Monitor infos, ``_dump_logs`` every    the chunk's ``done / ep_ret / ep_len`` records and the
``log_interval`` episodes              loss go to a pinned ring (64 chunks) by an async copy
                                       and are consumed once their event has completed: same
                                       episodes, same order, with that lag
callbacks: ``on_step`` per env step    ``on_rollout_start`` / ``on_rollout_end`` and ONE
                                       ``on_step`` per chunk, after ``num_timesteps`` advanced
                                       (the :class:`~imitation_amd.engine.rl.DevicePPO` convention)
=====================================  ==================================================

Eligible (:func:`supports`): a native vector env, the shapes of the fused TD step, ``train_freq``
of at most 16 steps, one rank, no ``VecNormalize``. The DQN object keeps its policy, buffers and
counters, so saving, prediction and host-side evaluation after ``learn`` work on it unchanged;
``learn`` ends by copying the device env state into the host env.
"""

from __future__ import annotations

import time
from typing import Any, Dict, List, Optional, Tuple

import numpy as np
import torch as th

from imitation_amd import ops
from imitation_amd.engine.generator import DeviceGeneratorCore, _unwrap_native
from imitation_amd.envs import spaces
from imitation_amd.envs.vec_env import VecNormalize, is_vecenv_wrapped
from imitation_amd.ops import dqn as td
from imitation_amd.parallel import dist as pdist
from imitation_amd.rl.dqn import DQN
from imitation_amd.rl.off_policy import polyak_update
from imitation_amd.rl.torch_layers import FlattenExtractor
from imitation_amd.utils.errflag import DeviceErrorFlag

RING = 64  # chunks of records in flight before the host waits for the oldest


def supports(venv, algorithm) -> Tuple[bool, str]:
    """Whether :class:`DeviceDQN` can train ``algorithm`` on ``venv`` (reason when not)."""
    if not isinstance(algorithm, DQN):
        return False, "learner is not DQN"
    nat = _unwrap_native(venv)
    if nat is None:
        return False, "env is not a native vector env"
    if nat._is_image:
        return False, "image observations"
    if algorithm.policy.features_extractor_class is not FlattenExtractor:
        return False, "Q-network is not a vector-observation MLP (CnnPolicy / MultiInputPolicy)"
    if not isinstance(nat.action_space, spaces.Discrete):
        return False, "env actions are not discrete"
    tf = algorithm.train_freq
    if tf.unit != "step":
        return False, f"train_freq counts {tf.unit}s, not steps"
    if not 1 <= tf.frequency <= td.MAX_COLLECT_STEPS:
        return False, (f"train_freq of {tf.frequency} steps (one launch collects at most {td.MAX_COLLECT_STEPS}; "
                       "larger values are not eligible yet)")
    if is_vecenv_wrapped(venv, VecNormalize) or algorithm._vec_normalize_env is not None:
        return False, "venv is wrapped in VecNormalize"
    if pdist.world_size() > 1:
        return False, "data parallel"
    if algorithm.optimize_memory_usage:
        return False, "optimize_memory_usage"
    if algorithm.action_noise is not None:
        return False, "action noise"
    if nat.num_envs != algorithm.n_envs:
        return False, "venv and learner disagree on the number of envs"
    if not th.cuda.is_available():
        return False, "no GPU"
    why = algorithm._td_ineligible(algorithm.batch_size)
    if why is not None:
        return False, f"the fused TD step does not apply ({why})"
    return True, ""


class DeviceDQN:
    """``algorithm.learn`` with the collection on the GPU (module docstring)."""

    def __init__(self, algorithm: DQN, venv, custom_logger=None) -> None:
        ok, why = supports(venv, algorithm)
        if not ok:
            raise ValueError(f"DeviceDQN not applicable: {why}; use DQN.learn")
        self.algo = algorithm
        self.venv = venv
        if custom_logger is not None:
            algorithm.set_logger(custom_logger)
        self._native = _unwrap_native(venv)
        self._C = ops.native()
        self._dev = algorithm.device
        self.N = self._native.num_envs
        self.K = int(algorithm.train_freq.frequency)
        self.D = int(np.prod(self._native.observation_space.shape))
        self.A = int(self._native.action_space.n)
        self.max_steps = int(self._native.max_episode_steps)
        algorithm.td_path = "fused"  # (supports: _td_ineligible is None)
        algorithm._td_bind()
        self.state = None  # (the env block is mirrored when learn starts)
        seed = algorithm.seed if algorithm.seed is not None else int(np.random.randint(0, 2**31 - 1))
        # the action streams: one per env, apart from the envs' own streams
        self.act_rng = td.action_streams((int(seed) * 0x2545F4914F6CDD1D + 0x5851F42D4C957F2D) & ((1 << 64) - 1), self.N,
                                         self._dev)
        rb = algorithm.replay_buffer
        # SQILReplayBuffer.add stores reward 0 whatever the env gave
        from imitation_amd.algorithms.sqil import SQILReplayBuffer

        self._reward_const = 0.0 if isinstance(rb, SQILReplayBuffer) else None
        # one device buffer per chunk: done [K, N], ep_ret [K, N], ep_len [K, N] (int32 bits), the mean
        # loss and the error word -- ONE async copy into the pinned ring
        KN = self.K * self.N
        self._rec_dev = th.zeros(3 * KN + 2, device=self._dev)
        self._rec = dict(done=self._rec_dev[:KN].view(self.K, self.N), ep_ret=self._rec_dev[KN : 2 * KN].view(self.K, self.N),
                         ep_len=self._rec_dev[2 * KN : 3 * KN].view(th.int32).view(self.K, self.N),
                         action=th.zeros(self.K, self.N, dtype=th.int64, device=self._dev))
        self._loss_dev = self._rec_dev[3 * KN : 3 * KN + 1]
        self._err = DeviceErrorFlag(self._dev, "DQN collect kernel")
        self._err.word = self._rec_dev[3 * KN + 1 :].view(th.int32)  # (rides along with the records)
        self._host = th.zeros(RING, 3 * KN + 2, pin_memory=True)
        self._events = [th.cuda.Event() for _ in range(RING)]
        self._pending: List[Tuple[int, bool]] = []  # (ring slot, the chunk trained) in launch order
        self._slot = 0
        self._log_interval: Optional[int] = None
        self._syncs_due = 0
        self._err_seen = 0
        self.n_target_syncs = 0

    # ------------------------------------------------------------------ the wrapped DQN's surface
    @property
    def logger(self):
        return self.algo.logger

    @property
    def policy(self):
        return self.algo.policy

    @property
    def num_timesteps(self) -> int:
        return self.algo.num_timesteps

    def save(self, *args, **kwargs):
        return self.algo.save(*args, **kwargs)

    def get_env(self):
        return self.algo.get_env()

    def predict(self, *args, **kwargs):
        return self.algo.predict(*args, **kwargs)

    # ------------------------------------------------------------------ env state
    def _mirror(self, obs0) -> None:
        """The host env block, just reset to ``obs0``, as device tensors."""
        env = DeviceGeneratorCore._env_mirror(self, self._native.get_state(), obs0)
        self.state, self.env_rng, self.elapsed = env["state"], env["rng"], env["elapsed"]
        self.ep_ret, self.cur_obs = env["ep_ret"], env["cur_obs"]

    def _env_tensors(self) -> Dict[str, Any]:
        """The env block as :func:`imitation_amd.ops.dqn.dqn_collect` takes it."""
        return dict(env=self._native.env_id, max_steps=self.max_steps, state=self.state, rng=self.env_rng,
                    elapsed=self.elapsed, ep_ret=self.ep_ret, cur_obs=self.cur_obs)

    def sync_env_to_host(self) -> None:
        """Copy the device env state back into the native host env (host-side evaluation / a host
        ``learn`` continue from the training env state)."""
        DeviceGeneratorCore.sync_env_to_host(self)
        self.algo._last_obs = self.cur_obs.cpu().numpy().reshape((self.N,) + tuple(self._native.observation_space.shape))

    def check_errors(self, blocking: bool = False) -> None:
        """Raise if any launch so far met a non-finite Q-value (non-blocking: as of the newest
        chunk of records the host has consumed)."""
        word = int(self._err.word.item()) if blocking else self._err_seen
        if word:
            from imitation_amd.utils.watchdog import NonFiniteError

            raise NonFiniteError("DQN collect kernel: non-finite Q-values (the online network is poisoned)")

    # ------------------------------------------------------------------ one chunk
    def _thresholds(self, total_timesteps: int) -> List[int]:
        """The chunk's ``K`` exploration thresholds, and the host loop's bookkeeping of those ``K``
        steps (``num_timesteps``, ``_n_calls``, ``exploration_rate``, target syncs due)."""
        algo = self.algo
        every = max(algo.target_update_interval // algo.n_envs, 1)
        eps: List[float] = []
        for _ in range(self.K):
            eps.append(1.0 if algo.num_timesteps < algo.learning_starts else algo.exploration_rate)
            algo.num_timesteps += self.N
            algo._update_current_progress_remaining(algo.num_timesteps, total_timesteps)
            algo._n_calls += 1
            if algo._n_calls % every == 0:
                self._syncs_due += 1
            algo.exploration_rate = algo.exploration_schedule(algo._current_progress_remaining)
        algo.logger.record("rollout/exploration_rate", algo.exploration_rate)
        return td.explore_thresholds(eps)

    def _sync_target(self) -> None:
        """The target syncs that fell into the chunk just launched (flat buckets: one copy)."""
        algo = self.algo
        n = algo._td["layout"].n
        for _ in range(self._syncs_due):
            if algo.tau >= 1.0:
                algo._td["target"][:n].copy_(algo.policy.optimizer._flat[0]["flat"][:n])
            else:
                polyak_update(algo.q_net.parameters(), algo.q_net_target.parameters(), algo.tau)
            self.n_target_syncs += 1
        self._syncs_due = 0

    def _consume(self, wait: bool) -> None:
        """Read the chunks whose copy has landed (all of them when ``wait``): Monitor's episode
        infos into ``ep_info_buffer``, ``_dump_logs`` every ``log_interval`` episodes, the loss."""
        algo = self.algo
        KN = self.K * self.N
        while self._pending:
            slot, trained = self._pending[0]
            ev = self._events[slot]
            if not ev.query():
                if not wait:
                    return
                ev.synchronize()
            self._pending.pop(0)
            h = self._host[slot].numpy()
            self._err_seen |= int(h[3 * KN + 1 :].view(np.int32)[0])
            if trained:
                loss = float(h[3 * KN])
                if not np.isfinite(loss):
                    from imitation_amd.utils.watchdog import NonFiniteError

                    raise NonFiniteError("non-finite DQN loss")
                algo.logger.record("train/n_updates", algo._n_updates, exclude="tensorboard")
                algo.logger.record("train/loss", loss)
            done = h[:KN].reshape(self.K, self.N) > 0.5
            if not done.any():
                continue
            ep_ret = h[KN : 2 * KN].reshape(self.K, self.N)
            ep_len = h[2 * KN : 3 * KN].view(np.int32).reshape(self.K, self.N)
            now = round((time.time_ns() - algo.start_time) / 1e9, 6)
            for t, n in zip(*(x.tolist() for x in np.nonzero(done))):  # completion order: step, then env
                algo.ep_info_buffer.append({"r": round(float(ep_ret[t, n]), 6), "l": int(ep_len[t, n]), "t": now})
                algo._episode_num += 1
                if self._log_interval is not None and algo._episode_num % self._log_interval == 0:
                    algo._dump_logs()

    def _chunk(self, total_timesteps: int) -> None:
        algo = self.algo
        rb = algo.replay_buffer
        algo._td_bind()  # (whatever rebound a parameter since the last chunk is packed again)
        thr = self._thresholds(total_timesteps)
        td.dqn_collect(self._env_tensors(), rb.td_fields(), rb.pos, rb.buffer_size, algo.policy.optimizer._flat[0]["flat"],
                       algo._td["layout"], thr, self.act_rng, reward_const=self._reward_const,
                       write_timeouts=rb.handle_timeout_termination, records=self._rec, err=self._err.word)
        pos = rb.pos + self.K
        if pos >= rb.buffer_size:
            rb.full = True
        rb.pos = pos % rb.buffer_size
        self._sync_target()
        trained = algo.num_timesteps > 0 and algo.num_timesteps > algo.learning_starts
        gs = algo.gradient_steps if algo.gradient_steps >= 0 else self.K * self.N
        trained = trained and gs > 0
        if trained:
            algo.policy.set_training_mode(True)
            algo._update_learning_rate(algo.policy.optimizer)
            losses = algo._td_launch(gs, algo.batch_size)
            algo._n_updates += gs
            th.mean(losses, dim=0, keepdim=True, out=self._loss_dev)
        # the records (and the loss) -> pinned ring; the host reads them when the event has completed
        if len(self._pending) == RING:
            self._consume_oldest()
        slot = self._slot
        self._slot = (slot + 1) % RING
        self._host[slot].copy_(self._rec_dev, non_blocking=True)
        self._events[slot].record()
        self._pending.append((slot, trained))
        self._consume(wait=False)
        self.check_errors()  # (the error word as of the newest chunk consumed; learn ends blocking)

    def _consume_oldest(self) -> None:
        self._events[self._pending[0][0]].synchronize()
        self._consume(wait=False)

    def learn(self, total_timesteps: int, callback=None, log_interval: Optional[int] = 4,
              reset_num_timesteps: bool = True, tb_log_name: str = "DQN", progress_bar: bool = False) -> "DeviceDQN":
        """``DQN.learn``: chunks of ``train_freq`` steps of every env until ``num_timesteps`` reaches
        ``total_timesteps``. ``callback`` (anything ``DQN.learn`` accepts; its model is the wrapped
        DQN) sees ``on_rollout_start`` / ``on_rollout_end`` and ONE ``on_step`` per chunk; an
        ``on_step`` returning False stops the training after that chunk."""
        algo = self.algo
        fresh = reset_num_timesteps or algo._last_obs is None
        total_timesteps, callback = algo._setup_learn(total_timesteps, callback, reset_num_timesteps, tb_log_name,
                                                      progress_bar)
        if fresh or self.state is None:
            # _setup_learn has just reset the host envs, or this is the engine's first learn on envs
            # the host loop has stepped: training starts from the host state
            self._mirror(algo._last_obs)
        self._log_interval = log_interval
        callback.on_training_start(locals(), globals())
        while algo.num_timesteps < total_timesteps:
            callback.on_rollout_start()
            self._chunk(total_timesteps)
            callback.on_rollout_end()
            if not callback.on_step():
                break
        self._consume(wait=True)
        callback.on_training_end()
        self.check_errors(blocking=True)
        self.sync_env_to_host()
        return self
