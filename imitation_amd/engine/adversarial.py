"""What the device GAIL and AIRL engines share (:class:`DeviceEngineMixin`): the replay store and
episode bookkeeping, the round scheduler, the graphed generic discriminator update and the driver
of the fused one. An engine (:mod:`imitation_amd.engine.gail`, :mod:`imitation_amd.engine.airl`)
supplies what differs between the two fused updates: ``_supports``, ``_fused_disc_check`` (its
limits, after ``_common_disc_check``), ``_setup_disc_plan`` (its nets, normalisers, workspace and
plan, on ``_setup_disc_params``) and ``_fused_disc_update`` (its merge flags, to ``_run_disc_update``).
"""

from __future__ import annotations

import collections
import os
import time
from typing import Any, Callable, Dict, List, Mapping, Optional, Sequence, Tuple

import numpy as np
import torch as th
from torch import nn

from imitation_amd.algorithms.adversarial import common
from imitation_amd.data import buffer as buffer_mod
from imitation_amd.engine.generator import DeviceGeneratorCore, _FlatParams
from imitation_amd.parallel import dist as pdist
from imitation_amd.rewards import reward_nets
from imitation_amd.rl.ppo import PPO
from imitation_amd.util import networks
from imitation_amd.utils import gcfreeze, profiling
from imitation_amd.utils.streams import shared_stream


def flatten_order(dones: np.ndarray, ep_lens_running: np.ndarray):
    """Replay order of one round's ``[T, N]`` transitions as BufferingWrapper -> flatten ->
    FIFO store produces it: finished episodes in completion order ((end step, env) row-major),
    each in time order, then every env's unfinished tail, by env. Vectorised (no Python loop
    over steps: this runs on the host between a rollout and its discriminator updates).

    Returns ``(order, fin_t, fin_n, ep_lens, ep_lens_running')``: flat row indices
    ``t * N + n``, the end step / env of each finished episode, its full length (including the
    steps carried from earlier rounds, ``ep_lens_running``) and the updated carry."""
    T, N = dones.shape
    ep_lens_running = np.asarray(ep_lens_running, dtype=np.int64)
    fin_t, fin_n = np.nonzero(dones)  # row-major: by end step, then env
    # episode starts: previous done of the same env + 1 (0 for its first done this round)
    by_env = np.lexsort((fin_t, fin_n))
    t_env, n_env = fin_t[by_env], fin_n[by_env]
    first = np.ones(len(by_env), dtype=bool)
    first[1:] = n_env[1:] != n_env[:-1]
    s_env = np.where(first, 0, np.concatenate(([0], t_env[:-1] + 1)))
    starts = np.empty_like(s_env)
    starts[by_env] = s_env
    is_first = np.empty_like(first)
    is_first[by_env] = first
    lens = fin_t - starts + 1
    ep_lens = (lens + np.where(is_first, ep_lens_running[fin_n], 0)).astype(np.int64)
    # tails: from the last done + 1 (or 0) to T - 1
    seg_start = np.zeros(N, dtype=np.int64)
    last = np.ones(len(by_env), dtype=bool)
    last[:-1] = n_env[:-1] != n_env[1:]
    seg_start[n_env[last]] = t_env[last] + 1
    done_any = np.zeros(N, dtype=bool)
    done_any[n_env] = True
    running = np.where(done_any, T - seg_start, ep_lens_running + T)
    tail_n = np.flatnonzero(seg_start < T)
    tail_s = seg_start[tail_n]
    # concatenated ranges [s, e] -> row indices, episodes first, then tails
    seg_s = np.concatenate((starts, tail_s))
    seg_len = np.concatenate((lens, T - tail_s))
    seg_env = np.concatenate((fin_n, tail_n))
    total = int(seg_len.sum())
    offs = np.repeat(np.cumsum(seg_len) - seg_len, seg_len)
    t_rows = np.repeat(seg_s, seg_len) + (np.arange(total) - offs)
    order = t_rows * N + np.repeat(seg_env, seg_len)
    return order.astype(np.int64), fin_t, fin_n, ep_lens.tolist(), running


class DeviceEngineMixin(DeviceGeneratorCore):
    """Device generator rounds (rollout -> GAE -> PPO -> replay store) and the fused
    discriminator update for an :class:`~imitation_amd.algorithms.adversarial.common.AdversarialTrainer`
    subclass; mixed in front of GAIL (:class:`imitation_amd.engine.gail.DeviceGAIL`) or AIRL
    (:class:`imitation_amd.engine.airl.DeviceAIRL`)."""

    _host_cls_name = "the host trainer"
    #: The updates queue behind PPO on the main stream (AIRL: log pi needs the post-PPO policy).
    _disc_on_main = False
    #: Split rounds (:meth:`_after_ppo` of an engine that has them).
    _disc_split = False

    def __init__(self, *, demonstrations, demo_batch_size: int, venv, gen_algo: PPO, reward_net: reward_nets.RewardNet, **kwargs):
        ok, why = self._supports(venv, gen_algo, reward_net)
        if not ok:
            raise ValueError(f"{type(self).__name__} not applicable: {why}; use {self._host_cls_name}")
        super().__init__(demonstrations=demonstrations, demo_batch_size=demo_batch_size, venv=venv, gen_algo=gen_algo,
                         reward_net=reward_net, **kwargs)
        self._init_generator(venv)
        D = self.D
        act_shape = () if self.discrete else (self.A,)
        self._gen_dev = buffer_mod.DeviceBuffer(
            self._gen_replay_buffer.capacity, {"obs": (D,), "acts": act_shape, "next_obs": (D,), "dones": ()},
            {"obs": th.float32, "acts": th.int64 if self.discrete else th.float32, "next_obs": th.float32,
             "dones": th.bool}, self._dev)
        # RewardVecEnvWrapper bookkeeping: None until the first round (_track_wrapped_returns)
        self._wrapped_eps = self._wrapped_cum = self._wrapped_mean_at_start = None
        self._disc_graph = self._disc_stats_gen = None  # _graphed_disc_update
        self._setup_fused_disc()

    @profiling.traced("host/replay_store")
    def _store_generator_samples(self) -> None:
        """Replay-buffer content identical to BufferingWrapper -> flatten -> FIFO store."""
        wrapped_rew = None
        if self._host_staged:
            dones = self._host_stage[0].numpy().astype(bool)
            ep_ret_host = self._host_stage[1].numpy()
            if self._host_stage.shape[0] == 4:
                wrapped_rew = self._host_stage[2].numpy() - self._host_stage[3].numpy()
            self._host_staged = False
        else:
            dones = self.buf["dones"].to("cpu", non_blocking=False).numpy().astype(bool)  # [T, N] (one sync / round)
            ep_ret_host = None
        T, N = dones.shape
        self._track_wrapped_returns(dones, wrapped_rew)
        order, fin_t, fin_n, ep_lens, self._ep_lens_running = flatten_order(dones, self._ep_lens_running)
        cap = self._gen_dev.capacity
        # pinned + non-blocking: a pageable H2D copy would block the host until the stream
        # reaches it (in an AIRL split round: until the PPO kernel ends, which left the round's
        # staging and the next step chain to be enqueued behind the GPU instead of ahead of it)
        keep = th.from_numpy(np.ascontiguousarray(order[-cap:])).pin_memory().to(self._dev, non_blocking=True)
        rows = T * N
        acts = self.buf["act_env"].reshape(rows, -1)
        if self.discrete:
            acts = acts.reshape(rows).long()
        self._gen_dev.store({
            "obs": self.buf["obs_buf"].reshape(rows, self.D).index_select(0, keep),
            "acts": acts.index_select(0, keep),
            "next_obs": self.buf["next_obs"].reshape(rows, self.D).index_select(0, keep),
            "dones": self.buf["dones"].reshape(rows).index_select(0, keep).bool(),
        })
        local_lens = list(ep_lens)
        if pdist.world_size() > 1 and not self.allow_variable_horizon:
            # global horizon set == {global min, global max}: one 2-float MIN all-reduce
            lo, neg_hi = pdist.allreduce_scalars([min(ep_lens, default=2**31), -max(ep_lens, default=-1)], op="min")
            ep_lens = [] if lo > -neg_hi else sorted({int(lo), int(-neg_hi)})
        self._check_fixed_horizon(ep_lens)
        # Monitor-style episode stats for the generator logger
        if len(fin_t):
            ep_ret = ep_ret_host if ep_ret_host is not None else self.buf["ep_ret_out"].cpu().numpy()
            algo = self.gen_algo
            if algo.ep_info_buffer is None:
                algo.ep_info_buffer = collections.deque(maxlen=algo._stats_window_size)
            for t, n, l_full in zip(fin_t.tolist(), fin_n.tolist(), local_lens):
                algo.ep_info_buffer.append({"r": float(ep_ret[t, n]), "l": int(l_full), "t": 0.0})

    def _track_wrapped_returns(self, dones: np.ndarray, rew: Optional[np.ndarray]) -> None:
        """``RewardVecEnvWrapper`` episode bookkeeping (reference ``rewards/reward_wrapper.py:15-37,
        92-133``): per-env running sums of the learned reward, a deque of the last 100 finished
        episodes' sums; ``rollout/ep_rew_wrapped_mean`` is its mean at the START of the rollout
        (``WrappedRewardCallback._on_rollout_start``), i.e. before this round's episodes."""
        # (getattr here and in engine_state: the CPU tests run both on stand-ins that __init__ did not set up)
        if getattr(self, "_wrapped_eps", None) is None:
            self._wrapped_eps = collections.deque(maxlen=100)
            self._wrapped_cum = np.zeros(dones.shape[1], dtype=np.float64)
        eps = self._wrapped_eps
        self._wrapped_mean_at_start = (sum(eps) / len(eps)) if eps else None
        if rew is None:
            return
        T, N = dones.shape
        cs = np.cumsum(rew.astype(np.float64), axis=0)  # [T, N] running sums within the round
        fin_t, fin_n = np.nonzero(dones)  # completion order: step, then env (the wrapper's loop)
        prev = np.full(N, -1, dtype=np.int64)
        vals = np.empty(len(fin_t), dtype=np.float64)
        for n in range(N):  # per env: segment sums between consecutive dones (+ the carry)
            sel = np.flatnonzero(fin_n == n)
            if not len(sel):
                continue
            t = fin_t[sel]
            before = np.concatenate(([0.0], cs[t[:-1], n]))
            v = cs[t, n] - before
            v[0] += self._wrapped_cum[n]
            vals[sel] = v
            prev[n] = t[-1]
        eps.extend(vals.tolist())
        last = np.where(prev >= 0, cs[T - 1] - np.where(prev >= 0, cs[np.maximum(prev, 0), np.arange(N)], 0.0),
                        self._wrapped_cum + cs[T - 1])
        self._wrapped_cum = last

    def _gen_sample(self, batch_size: int) -> Dict[str, th.Tensor]:
        if self._gen_dev.size() == 0:
            raise RuntimeError("No generator samples for training. Call `train_gen()` first.")
        return self._gen_dev.sample(batch_size)

    def train_gen(self, total_timesteps: Optional[int] = None, learn_kwargs: Optional[Mapping] = None) -> None:
        """One (or more) device rounds: rollout -> GAE -> PPO update -> replay store."""
        if total_timesteps is None:
            total_timesteps = self.gen_train_timesteps
        algo: PPO = self.gen_algo
        n_rounds = max(1, total_timesteps // (self.T * self.N))
        with self.logger.accumulate_means("gen"):
            for _ in range(n_rounds):
                if algo._total_timesteps < algo.num_timesteps + self.T * self.N:
                    algo._total_timesteps = algo.num_timesteps + self.T * self.N
                self._rollout()
                # episode bookkeeping needs dones / returns on the host: copy them right after
                # the rollout and let the CPU work while the PPO kernel runs
                ready = self._stage_rollout_to_host()
                algo.num_timesteps += self.T * self.N
                self._ppo_update()
                ready.synchronize()
                self._store_generator_samples()
                self._global_step += 1
            self._log_gen()

    @profiling.traced("host/log_gen")
    def _log_gen(self) -> None:
        """Record one generator round with the host trainer's key set: SB3 ``PPO.train`` metrics
        (:meth:`_ppo_log_values`), ``OnPolicyAlgorithm._dump_logs`` (``time/*``, Monitor
        ``rollout/ep_*_mean``) and the reward wrapper's ``rollout/ep_rew_wrapped_mean``
        (reference ``adversarial/common.py:234-240, 414-419``). ``time/fps``: env steps per
        second of wall time since the previous round's record (the round's sustained rate; the
        reference's per-round ``learn`` call gives the same quantity)."""
        self._record_round_metrics()
        if self._wrapped_mean_at_start is not None:
            self.logger.record("rollout/ep_rew_wrapped_mean", float(self._wrapped_mean_at_start))

    # ------------------------------------------------------------------ fused discriminator update: setup
    def _common_disc_check(self, host_cls) -> Tuple[bool, str]:
        """What both fused updates need (``host_cls``: the trainer whose logits the kernels compute)."""
        if type(self).logits_expert_is_high is not host_cls.logits_expert_is_high:
            return False, "custom discriminator logits"
        opt = self._disc_opt
        if type(opt) is not th.optim.Adam or len(opt.param_groups) != 1:
            return False, "discriminator optimizer is not a single-group torch.optim.Adam"
        g = opt.param_groups[0]
        if any(g.get(k) for k in ("amsgrad", "maximize", "capturable", "differentiable", "decoupled_weight_decay")):
            return False, "Adam variant not fused"
        if self._init_tensorboard:
            return False, "tensorboard summaries need per-step logits"
        if not isinstance(self._endless_expert_iterator, common._DeviceDemoSampler):
            return False, "demonstrations are not a flat device transitions set"
        return True, ""

    def _reward_params_are(self, lins: Sequence[nn.Linear]) -> bool:
        """The reward net trains the weights and biases of ``lins`` and nothing else."""
        return {id(p) for p in self._reward_net.parameters()} == {id(p) for l in lins for p in (l.weight, l.bias)}

    def _setup_fused_disc(self) -> None:
        ok, why = self._fused_disc_check()
        self._fused_disc = ok
        self._fused_disc_why = why
        # Overlap (see _overlapped_round): GAIL's updates of a round run on a side stream,
        # concurrently with its PPO update; AIRL's follow PPO on the main stream (_disc_on_main) and
        # the side stream carries the rollout's staging copies (also when the update is not fused)
        # and the applies of split rounds. IMITATION_AMD_DISC_OVERLAP=0: serial rounds.
        self._overlap_disc = os.environ.get("IMITATION_AMD_DISC_OVERLAP", "1") != "0"
        if self._overlap_disc and (ok or self._disc_on_main):
            self._side_stream = shared_stream(self._dev, "engine_side")
        self._pol_defer_buf = None  # (_ensure_pol_defer)
        if ok:
            self._setup_disc_plan()

    def _setup_disc_params(self, lins: Sequence[nn.Linear]) -> Dict[str, th.Tensor]:
        """The parameters of ``lins`` in one flat buffer with their Adam moments (adopted by the
        optimizer) and the statistics buffers; returns the expert set in the gather kernels' layout."""
        self._rflat = _FlatParams([p for l in lins for p in (l.weight, l.bias)])
        self._r_m = th.zeros(self._rflat.n, device=self._dev)
        self._r_v = th.zeros(self._rflat.n, device=self._dev)
        self._adopt_disc_opt_state()
        self._alloc_disc_stats(max(1, self.n_disc_updates_per_round))
        ed = self._endless_expert_iterator.data
        ed["obs"] = ed["obs"].float().contiguous()
        ed["next_obs"] = ed["next_obs"].float().contiguous()
        ed["acts"] = (ed["acts"].long() if self.discrete else ed["acts"].float()).reshape(ed["acts"].shape[0], -1)
        ed["acts"] = ed["acts"].reshape(-1).contiguous() if self.discrete else ed["acts"].contiguous()
        ed["dones"] = ed["dones"].bool().contiguous()
        return ed

    def _alloc_disc_stats(self, n_updates: int) -> None:
        """One row of statistics sums per update of a round, and its pinned host copy."""
        self._disc_stats = th.zeros(n_updates, 8, device=self._dev)
        self._disc_stats_host = th.zeros(n_updates, 8, pin_memory=True)

    def _ensure_pol_defer(self, n_updates: int) -> None:
        """Room for the deferred policy-norm merges of ``n_updates`` updates (GAIL's plan)."""
        slots = n_updates * self._disc_plan.n_minibatches
        if self._pol_defer_buf is None or self._pol_defer_buf.shape[0] < slots:
            self._pol_defer_buf = th.zeros(slots, 2 * self._disc_plan.pol_cols + 1, device=self._dev)
            self._disc_plan.set_pol_defer(self._pol_defer_buf)

    def _adopt_disc_opt_state(self) -> None:
        """Make the torch Adam state of every reward parameter a view of the flat moment
        buffers the fused kernel updates (copying in any state the optimizer already has,
        e.g. after ``load_state_dict``), so both update paths and checkpoints agree."""
        opt = self._disc_opt
        for p, off in zip(self._rflat.params, self._rflat.offsets):
            k = p.numel()
            m = self._r_m[off : off + k].view_as(p)
            v = self._r_v[off : off + k].view_as(p)
            st = opt.state.get(p)
            if st and st.get("exp_avg") is not None and st["exp_avg"].data_ptr() == m.data_ptr() \
                    and st["exp_avg_sq"].data_ptr() == v.data_ptr():
                continue
            step = th.tensor(0.0)
            if st:
                with th.no_grad():
                    m.copy_(st["exp_avg"])
                    v.copy_(st["exp_avg_sq"])
                step = st["step"] if isinstance(st["step"], th.Tensor) else th.tensor(float(st["step"]))
            else:
                m.zero_()
                v.zero_()
            opt.state[p] = {"step": step, "exp_avg": m, "exp_avg_sq": v}

    # ------------------------------------------------------------------ fused discriminator update: driver
    def _adam_scalars(self, ahead: int = 1) -> Tuple[float, float]:
        """Adam's (lr / (1 - beta1^t), sqrt(1 - beta2^t)) of the optimizer's ``ahead``-th step from
        now (after :meth:`_adopt_disc_opt_state`)."""
        g = self._disc_opt.param_groups[0]
        beta1, beta2 = g["betas"]
        t = float(self._disc_opt.state[self._rflat.params[0]]["step"]) + ahead
        return float(g["lr"]) / (1.0 - beta1**t), (1.0 - beta2**t) ** 0.5

    def _draw_disc_indices(self, e_idx: Optional[th.Tensor] = None, g_idx: Optional[th.Tensor] = None):
        """Expert and replay rows of one update, drawn in the host trainer's order (those given are kept)."""
        if self._gen_dev.size() == 0:
            raise RuntimeError("No generator samples for training. Call `train_gen()` first.")
        if e_idx is None:
            e_idx = self._endless_expert_iterator.next_indices()
        if g_idx is None:
            g_idx = th.randint(0, self._gen_dev.size(), (self.demo_batch_size,), device=self._dev)
        return e_idx, g_idx

    def _bump_disc_step(self) -> None:
        for p in self._rflat.params:
            self._disc_opt.state[p]["step"] += 1
        self._disc_step += 1

    def _run_disc_update(self, slot: int, merges: Tuple[bool, ...], e_idx: Optional[th.Tensor] = None,
                         g_idx: Optional[th.Tensor] = None, apply: bool = True, pol_slot: Optional[int] = None) -> None:
        """One discriminator optimizer step on the engine's plan with no host sync; statistics
        into row ``slot``. ``merges``: which RunningNorms merge the batch, in the plan's order.
        One rank: one launch. Data parallel, per minibatch: gather, batch moments, their
        all-reduce, the merges, forward / backward; then the gradient reduction, its mean over
        ranks and Adam. ``apply=False`` stops in that order after the gradient.
        ``pol_slot`` (GAIL's plan): the plan takes, last, the slot of the deferred-merge buffer
        that records the first minibatch's policy-norm merge (-1: merge in place), and nothing is
        launched for the norms when none merges. None (AIRL's plan): no such argument."""
        self._adopt_disc_opt_state()
        step_size, bc2_sqrt = self._adam_scalars()
        e_idx, g_idx = self._draw_disc_indices(e_idx, g_idx)
        plan = self._disc_plan
        stats_out = self._disc_stats[slot]
        world = pdist.world_size()
        if world == 1 and apply:
            ds = () if pol_slot is None else (pol_slot,)
            plan.update(e_idx, g_idx, step_size, bc2_sqrt, *merges, stats_out, *ds)
        else:
            mb = self.demo_minibatch_size
            for k in range(self.demo_batch_size // mb):
                plan.gather(k, e_idx, g_idx)
                if pol_slot is None or any(merges):
                    ds = () if pol_slot is None else (pol_slot + k if pol_slot >= 0 else -1,)
                    if pdist.norm_sync_active():
                        plan.norm(1, 0, *merges)
                        pdist.allreduce_sum_(self._disc_ws["sums"])
                        plan.norm(2, 2 * mb * world, *merges, *ds)
                    else:
                        plan.norm(0, 0, *merges, *ds)
                plan.fwd_bwd(k)
            plan.adam(1, 0, 0.0, 1.0, stats_out)
            if world > 1:
                pdist.allreduce_grads_flat(self._disc_ws["grads"])
            if not apply:
                return
            plan.adam(0, 1, step_size, bc2_sqrt, None)
        self._bump_disc_step()

    def _disc_stats_dict(self, v: Sequence[float]) -> Mapping[str, float]:
        B, mb = self.demo_batch_size, self.demo_minibatch_size
        rows = 2 * mb
        return common.train_stats_from_sums(
            [v[0] / rows * (mb / B), v[1] / rows, float(mb), v[2], v[3], v[4], v[5] / rows], float(rows))

    @profiling.traced("host/log_disc")
    def _record_disc(self, stats: Mapping[str, float], disc_step: int) -> None:
        self.logger.record("global_step", self._global_step)
        for k, v in stats.items():
            self.logger.record(k, v)
        self.logger.dump(disc_step)

    def _finish_disc_round(self, r: int, vals: Sequence[Sequence[float]], steps: Sequence[int], n_sums: int,
                           to_stats: Callable[[Sequence[float]], Mapping[str, float]], what: str, callback) -> None:
        """The host's end of round ``r``: fail on a lost peer or a non-finite sum (the first
        ``n_sums`` of each update's row in ``vals``), log every update as the reference's
        ``train_disc`` does, run the callback, dump the round's records."""
        pdist.check_comm(what)
        self._fail_if_nonfinite({f"update {i} sum {j}": float(v) for i, row in enumerate(vals)
                                 for j, v in enumerate(row[:n_sums])}, "discriminator")
        for row, step in zip(vals, steps):
            with self.logger.accumulate_means("disc"):
                self._record_disc(to_stats(row), step)
        if callback:
            callback(r)
        self.logger.dump(self._global_step)

    def train_disc(self, *, expert_samples: Optional[Mapping] = None, gen_samples: Optional[Mapping] = None) -> Mapping[str, float]:
        if not self._fused_disc or expert_samples is not None or gen_samples is not None:
            return super().train_disc(expert_samples=expert_samples, gen_samples=gen_samples)
        with self.logger.accumulate_means("disc"):
            self._fused_disc_update(0)
            stats = self._disc_stats_dict(self._disc_stats[0].tolist())
            self._record_disc(stats, self._disc_step)
        return stats

    # ------------------------------------------------------------------ graphed generic discriminator update
    def _graphed_disc_ok(self) -> bool:
        """The generic (autograd) discriminator step -- e.g. AIRL's shaped reward net, which
        the fused kernels do not cover -- as one HIP-graph replay per update: single
        process (no gradient all-reduce / norm collectives), a capturable optimiser, the
        device demo sampler, and no per-step tensorboard summaries (a host sync)."""
        from imitation_amd.utils import graphs

        # under DP the gradient mean and the normaliser moments go through the one-shot
        # all-reduce kernel, which a graph can hold (RCCL / gloo collectives cannot)
        single = pdist.world_size() == 1 and self._disc_bucket is None
        return (not self._fused_disc and (single or pdist.oneshot_active())
                and graphs.graphs_enabled(self._dev, "IMITATION_AMD_DISC_GRAPH")
                and graphs.supports_capture(self._disc_opt) and not self._init_tensorboard
                and isinstance(self._endless_expert_iterator, common._DeviceDemoSampler))

    def _generic_disc_fn(self, e_obs, e_acts, e_next, e_dones, g_idx) -> th.Tensor:
        """``AdversarialTrainer.train_disc``'s minibatch losses, backward and optimiser step
        over device batches (expert rows given, generator rows gathered from the device replay
        buffer by ``g_idx``); returns the last minibatch's statistics sums (device)."""
        import torch.nn.functional as F

        from imitation_amd.ops import optim as optim_ops
        from imitation_amd.ops.rl import gather_rows

        ga = self._gen_dev._arrays
        keys = ("obs", "acts", "next_obs", "dones")
        gen = dict(zip(keys, gather_rows([ga[k] for k in keys], g_idx)))  # one launch
        ex = {"obs": e_obs, "acts": e_acts, "next_obs": e_next, "dones": e_dones}
        # a single minibatch per update (the tuned configs): its gradients go straight into
        # FusedAdam's (zeroed) bucket, no accumulate-add per parameter
        into_buckets = (isinstance(self._disc_opt, optim_ops.FusedAdam)
                        and self.demo_minibatch_size == self.demo_batch_size)
        for batch in self._make_disc_train_batches(gen_samples=gen, expert_samples=ex):
            logits = self.logits_expert_is_high(batch["state"], batch["action"], batch["next_state"], batch["done"],
                                                batch["log_policy_act_prob"])
            loss = F.binary_cross_entropy_with_logits(logits, batch["labels_expert_is_one"].float())
            loss = loss * (self.demo_minibatch_size / self.demo_batch_size)
            if into_buckets:
                self._disc_opt.backward_into_buckets(loss)
            else:
                loss.backward()
        if pdist.world_size() > 1:  # mean over ranks of the flat bucket(s): one-shot, in-graph
            pdist.FlatGradBucket(self._disc_opt).allreduce()
        self._disc_opt.step()
        return common.train_stats_vec(logits, batch["labels_expert_is_one"], loss)

    def _graphed_disc_update(self, slot: int) -> None:
        from imitation_amd.utils import graphs

        if self._gen_dev.size() == 0:
            raise RuntimeError("No generator samples for training. Call `train_gen()` first.")
        if self._disc_graph is None:
            # torch Adam's capturable step is ~30 multi-tensor launches; the flat-bucket
            # FusedAdam (same hyper-parameters and state) is one
            from imitation_amd.ops import optim as optim_ops

            self._disc_opt = optim_ops.to_fused(self._disc_opt)
            self._disc_graph = graphs.GraphedTrainStep(self._generic_disc_fn, self._disc_opt)
        ex = self._next_expert_batch()
        g_idx = th.randint(0, self._gen_dev.size(), (self.demo_batch_size,), device=self._dev)
        out = self._disc_graph(ex["obs"], ex["acts"], ex["next_obs"], ex["dones"], g_idx)
        self._disc_stats_gen[slot].copy_(out)
        self._disc_step += 1

    def _train_graphed_generic(self, total_timesteps: int, callback=None) -> None:
        n_rounds = total_timesteps // self.gen_train_timesteps
        assert n_rounds >= 1, (
            f"No updates (need at least {self.gen_train_timesteps} timesteps, have only total_timesteps={total_timesteps})!")
        n = self.n_disc_updates_per_round
        if self._disc_stats_gen is None or self._disc_stats_gen.shape[0] < n:
            self._disc_stats_gen = th.zeros(max(n, 1), 7, device=self._dev)
        rows = float(2 * self.demo_minibatch_size)
        for r in range(n_rounds):
            self.train_gen(self.gen_train_timesteps)
            steps = []
            with networks.training(self.reward_train):
                for i in range(n):
                    self._graphed_disc_update(i)
                    steps.append(self._disc_step)
            vals = self._disc_stats_gen[:n].tolist() if n else []  # one host sync per round
            self._finish_disc_round(r, vals, steps, 7, lambda v: common.train_stats_from_sums(v, rows),
                                    "adversarial round", callback)
        self.check_errors(blocking=True)

    # ------------------------------------------------------------------ rounds
    #: Keep the round pipeline when ``train`` is given a callback: round ``r + 1``'s rollout
    #: (chain + reward pass) is already enqueued when ``callback(r)`` runs. The callback sees
    #: round ``r``'s final weights and may read (e.g. checkpoint) any state; it must not mutate
    #: the env state, the policy or the reward net in place (the in-flight rollout reads them).
    #: The CLI's checkpoint callback (reference ``scripts/train_adversarial.py:156-160``) only
    #: saves. False: every callback runs with the device idle, as a host-loop trainer would.
    pipeline_callbacks = True

    @gcfreeze.during
    def train(self, total_timesteps: int, callback=None) -> None:
        """Rounds of device generator training + fused discriminator updates; the
        discriminator statistics of a round are fetched with one host sync and logged
        per update exactly as the reference's ``train_disc`` does. At the end the host env
        mirrors the device env state: a host-side evaluation on ``venv_train`` (the reference
        CLI's final ``eval_policy``, e.g. AIRL with output normalisation) then continues from
        the training env state, as the reference's does, whether or not a checkpoint or a
        resume copied it before."""
        if not self._fused_disc:
            if self._graphed_disc_ok():
                self._train_graphed_generic(total_timesteps, callback)
            else:
                super().train(total_timesteps, callback)
        else:
            self._train_fused(total_timesteps, callback)
        self.sync_env_to_host()

    def _train_fused(self, total_timesteps: int, callback=None) -> None:
        n_rounds = total_timesteps // self.gen_train_timesteps
        assert n_rounds >= 1, (
            f"No updates (need at least {self.gen_train_timesteps} timesteps, have only total_timesteps={total_timesteps})!")
        n = self.n_disc_updates_per_round
        if n > self._disc_stats.shape[0]:
            self._alloc_disc_stats(n)
        overlap = self._overlap_disc and n > 0 and self.gen_train_timesteps == self.T * self.N
        nxt = None
        self._fps_mark = (time.perf_counter(), self.gen_algo.num_timesteps)
        timer = profiling.StepTimer(roctx=False)
        timer.n0 = self.gen_algo.num_timesteps
        for r in range(n_rounds):
            if overlap:
                # the next rollout is enqueued before this round's logging and callback (see
                # pipeline_callbacks), so the device never waits for the host between rounds
                launch = r + 1 < n_rounds and (callback is None or self.pipeline_callbacks)
                steps, nxt = self._overlapped_round(n, nxt, launch_next=launch)
                vals = self._disc_stats_host[:n].tolist()
            else:
                self.train_gen(self.gen_train_timesteps)
                steps = []
                with networks.training(self.reward_train):
                    for i in range(n):
                        self._fused_disc_update(i)
                        steps.append(self._disc_step)
                vals = self._disc_stats[:n].tolist() if n else []
            self._finish_disc_round(r, vals, steps, 6, self._disc_stats_dict, "GAIL round", callback)
        pdist.check_comm("GAIL training", blocking=True)
        self.check_errors(blocking=True)
        self._report_throughput(timer)

    def _report_throughput(self, timer: "profiling.StepTimer") -> None:
        """Per-rank and whole-node env-steps/s of this ``train`` call: host wall
        time of the call (its rounds are pipelined, so this is the sustained rate), one small
        all-reduce under DP. Recorded as ``perf/*`` and kept in ``last_train_perf``."""
        timer.add_env_steps(self.gen_algo.num_timesteps - timer.n0)
        rep = timer.report()
        self.last_train_perf = rep
        for k in ("rank_env_steps_per_s", "node_env_steps_per_s", "elapsed_s", "world_size"):
            self.logger.record(f"perf/{k}", rep[k])
        self.logger.dump(self._global_step)

    def _launch_rollout(self) -> th.cuda.Event:
        """Enqueue one rollout (chain + post pass) and the async copy of its dones / returns to
        pinned host memory; returns the event that marks both done."""
        self._rollout()
        return self._stage_rollout_to_host()

    def _overlapped_round(self, n: int, ready: Optional[th.cuda.Event] = None,
                          launch_next: bool = False) -> Tuple[List[int], Optional[th.cuda.Event]]:
        """One round pipelined with the next: the rollout, the PPO update, and then
        :meth:`_after_ppo` with the round's ``n`` discriminator updates.

        ``ready``: the round's rollout was already enqueued (by the previous call) and this
        is its staging event. ``launch_next``: enqueue the next round's rollout behind this
        round's device work BEFORE waiting for PPO on the host, so the GPU never idles while
        the host logs. Returns (disc steps, next round's staging event); the disc stats are in
        ``_disc_stats_host`` when this returns."""
        algo: PPO = self.gen_algo
        defer_pol = self.pol_norm is not None and self.pol_norm.training and self._pol_defer_buf is not None
        if defer_pol:
            self._ensure_pol_defer(n)
        with self.logger.accumulate_means("gen"):
            if algo._total_timesteps < algo.num_timesteps + self.T * self.N:
                algo._total_timesteps = algo.num_timesteps + self.T * self.N
            if ready is None:
                ready = self._launch_rollout()
            algo.num_timesteps += self.T * self.N
            self._ppo_update()
            ready.synchronize()
            return self._after_ppo(n, ready, launch_next, defer_pol)

    def _after_ppo(self, n: int, ready: th.cuda.Event, launch_next: bool, defer_pol: bool):
        """Rest of an overlapped round once PPO is enqueued and the rollout's dones are on the
        host: the replay store and the updates on the side stream, concurrent with the PPO update
        (the round's rewards were already computed from the previous discriminator, so nothing
        PPO reads changes); with ``_disc_on_main`` behind PPO on the main stream -- the round is
        still pipelined: nothing waits on the host between PPO, the updates and the next rollout.
        ``defer_pol``: the updates record their policy-norm merges -- the one write the PPO kernel
        also makes (GAIL's log-prob side effect) -- per minibatch, and they are applied in order
        after PPO, so the result is bitwise that of the serial order."""
        main = th.cuda.current_stream(self._dev)
        side = main if self._disc_on_main else self._side_stream
        ppo_done = self._ppo_done
        pol_merge = self.pol_norm is not None and self.pol_norm.training
        # serial when the disc would write the norm PPO is using, or when both would issue
        # per-step collectives: the non-replicated DP PPO all-reduces every minibatch through
        # the same one-shot communicator as the disc, and two kernels in flight on it would
        # pair one rank's PPO gradients with another rank's disc sums
        serial = (pol_merge and not defer_pol) or (pdist.world_size() > 1 and not self._dp_replicated)
        steps: List[int] = []
        nxt = None
        if serial:
            self._wait_ev(side, ppo_done)
        else:
            side.wait_event(ready)
        with th.cuda.stream(side):
            self._store_generator_samples()
            with networks.training(self.reward_train):
                for i in range(n):
                    self._fused_disc_update(i, defer_pol=defer_pol)
                    steps.append(self._disc_step)
            disc_dev = self._dev_event(side)
            self._disc_stats_host[:n].copy_(self._disc_stats[:n], non_blocking=True)
            disc_done = th.cuda.Event()
            disc_done.record(side)
        self._wait_ev(main, disc_dev)
        if defer_pol:
            self._disc_plan.pol_norm_merge(n * self._disc_plan.n_minibatches)
        self._global_step += 1
        if launch_next:
            nxt = self._launch_rollout()
        ppo_done.synchronize()
        self._log_gen()
        disc_done.synchronize()
        return steps, nxt

    # ------------------------------------------------------------------ checkpoint / resume
    def engine_state(self) -> Dict[str, Any]:
        """Device-engine state not covered by module ``state_dict``s (used by
        :mod:`imitation_amd.utils.checkpoint`); parameters live in the policy modules."""
        st = self._core_engine_state()
        if getattr(self, "_wrapped_eps", None) is not None:
            st["wrapped_eps"] = th.tensor(list(self._wrapped_eps), dtype=th.float64)
            st["wrapped_cum"] = th.as_tensor(self._wrapped_cum, dtype=th.float64)
        st.update(ep_lens_running=th.as_tensor(self._ep_lens_running),
                  gen_dev={k: v.cpu().clone() for k, v in self._gen_dev._arrays.items()},
                  gen_dev_idx=int(self._gen_dev._idx), gen_dev_n=int(self._gen_dev._n_data))
        return st

    def load_engine_state(self, st: Dict[str, Any]) -> None:
        self._load_core_engine_state(st)
        with th.no_grad():
            for k, v in st["gen_dev"].items():
                self._gen_dev._arrays[k].copy_(v.to(self._dev))
        self._ep_lens_running = st["ep_lens_running"].numpy().copy()
        if "wrapped_eps" in st:
            self._wrapped_eps = collections.deque(st["wrapped_eps"].tolist(), maxlen=100)
            self._wrapped_cum = st["wrapped_cum"].numpy().copy()
        self._gen_dev._idx, self._gen_dev._n_data = st["gen_dev_idx"], st["gen_dev_n"]
        self.sync_env_to_host()
