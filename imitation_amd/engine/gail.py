"""Device-resident adversarial imitation (GAIL / AIRL-ready) -- the MI355X fast path.

Same algorithm, hyper-parameters and public surface as
:class:`imitation_amd.algorithms.adversarial.gail.GAIL` (reference
``src/imitation/algorithms/adversarial/{common,gail}.py``), but a training round
never leaves the GPU:

=====================  ==========================================================
reference (host loop)  this engine
=====================  ==========================================================
SB3 collect_rollouts:  ``engine_rollout`` -- ONE kernel runs n_steps x n_envs of
policy fwd, VecEnv     policy sampling, env physics (native model) and the
pipes, reward wrapper  TimeLimit bootstrap; buffers are written straight into
numpy<->device copies  HBM. The learned reward ``softplus(D(s,a))`` does not feed
                       back into the dynamics: ``engine_reward_batch`` computes it
                       for all T x N transitions in one parallel pass afterwards
RolloutBuffer GAE      ``gae`` kernel (one lane per env)
(python loop)
PPO.train              ``engine_ppo_update`` -- ONE persistent workgroup runs all
(~10 launches / mb)    epochs x minibatches (fp32 MFMA, params in LDS, Adam in L2)
BufferingWrapper +     device replay ring, same FIFO content as the reference's
ReplayBuffer (numpy)   flatten-then-store order
train_disc             fused MLP fwd/bwd kernels + device demo sampler
=====================  ==========================================================

Data parallel: each rank runs its own envs; the PPO update switches to the
per-minibatch kernel pair with an RCCL all-reduce of the normaliser moments and
of the flat gradient between them (synchronous DP == large-batch SGD), and the
discriminator averages its gradient bucket once per update.

Eligibility (checked in :func:`supports`): native vector env (non-image), an
on-policy :class:`~imitation_amd.rl.ppo.PPO` with an MLP actor-critic (widths ≤ 64,
≤ 4 layers, minibatch ≤ 128 and a multiple of 16), and an MLP
``BasicRewardNet`` (optionally inside ``NormalizedRewardNet``). Anything else
should use the host-loop trainers.

The generator rows of the table (rollout, GAE, PPO update, with the data-parallel plan) are
:class:`imitation_amd.engine.generator.DeviceGeneratorCore`, shared with the preference-comparison
and ``train_rl`` engines; this module adds the replay store and the discriminator rounds.
"""

from __future__ import annotations

import collections
import os
import time
from typing import Any, Dict, List, Mapping, Optional, Sequence, Tuple

import numpy as np
import torch as th
from torch import nn

from imitation_amd.algorithms.adversarial import common
from imitation_amd.algorithms.adversarial.gail import GAIL
from imitation_amd.data import buffer as buffer_mod
from imitation_amd.engine.generator import DeviceGeneratorCore, _FlatParams, _mlp_layers, _split, supports_generator
from imitation_amd.parallel import dist as pdist
from imitation_amd.rewards import reward_nets
from imitation_amd.rl.ppo import PPO
from imitation_amd.util import networks
from imitation_amd.utils import gcfreeze, profiling
from imitation_amd.utils.streams import shared_stream


def supports(venv, gen_algo, reward_net) -> Tuple[bool, str]:
    """Whether :class:`DeviceGAIL` can run this configuration (reason when not)."""
    ok, why = supports_generator(venv, gen_algo)
    if not ok:
        return ok, why
    if not isinstance(_split(reward_net)[1], reward_nets.BasicRewardNet):
        return False, "reward net is not a BasicRewardNet"
    return True, ""


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
    subclass; mixed in front of GAIL (:class:`DeviceGAIL`) or AIRL
    (:class:`imitation_amd.engine.airl.DeviceAIRL`)."""

    _host_cls_name = "the host trainer"

    @staticmethod
    def _supports(venv, gen_algo, reward_net) -> Tuple[bool, str]:
        return supports(venv, gen_algo, reward_net)

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
    def _log_gen(self, stats: Optional[th.Tensor] = None) -> None:
        """Record one generator round with the host trainer's key set: SB3 ``PPO.train`` metrics
        (:meth:`_ppo_log_values`), ``OnPolicyAlgorithm._dump_logs`` (``time/*``, Monitor
        ``rollout/ep_*_mean``) and the reward wrapper's ``rollout/ep_rew_wrapped_mean``
        (reference ``adversarial/common.py:234-240, 414-419``). ``time/fps``: env steps per
        second of wall time since the previous round's record (the round's sustained rate; the
        reference's per-round ``learn`` call gives the same quantity). ``stats`` is unused (kept
        for callers that pass the old host copy)."""
        self._record_round_metrics()
        wm = getattr(self, "_wrapped_mean_at_start", None)
        if wm is not None:
            self.logger.record("rollout/ep_rew_wrapped_mean", float(wm))

    # ------------------------------------------------------------------ fused discriminator update
    def _fused_disc_check(self) -> Tuple[bool, str]:
        if type(self).logits_expert_is_high is not GAIL.logits_expert_is_high:
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
        _, base = _split(self._reward_net)
        try:
            norm, lins, _, out_act = _mlp_layers(base.mlp)
        except ValueError as e:
            return False, str(e)
        if norm is not None and type(norm) is not networks.RunningNorm:
            return False, "reward-net input normaliser is not RunningNorm"
        if out_act != 0 or lins[-1].out_features != 1 or len(lins) > 4:
            return False, "reward MLP shape"
        if max([lins[0].in_features] + [l.out_features for l in lins]) > 128:
            return False, "reward MLP wider than 128"
        mlp_params = {id(p) for l in lins for p in (l.weight, l.bias)}
        if {id(p) for p in self._reward_net.parameters()} != mlp_params:
            return False, "reward net has parameters outside its MLP"
        if self.pol_norm is not None and (type(self.pol_norm) is not networks.RunningNorm or not base.use_state):
            return False, "policy normaliser"
        return True, ""

    def _setup_fused_disc(self) -> None:
        ok, why = self._fused_disc_check()
        self._fused_disc = ok
        self._fused_disc_why = why
        if not ok:
            return
        dev = self._dev
        _, base = _split(self._reward_net)
        norm, lins, hid, _ = _mlp_layers(base.mlp)
        self._rnorm = norm
        plist: List[nn.Parameter] = []
        for l in lins:
            plist += [l.weight, l.bias]
        self._rflat = _FlatParams(plist)
        n = self._rflat.n
        self._r_m = th.zeros(n, device=dev)
        self._r_v = th.zeros(n, device=dev)
        self._adopt_disc_opt_state()
        sampler = self._endless_expert_iterator
        ed = sampler.data
        ed["obs"] = ed["obs"].float().contiguous()
        ed["next_obs"] = ed["next_obs"].float().contiguous()
        ed["acts"] = (ed["acts"].long() if self.discrete else ed["acts"].float()).reshape(ed["acts"].shape[0], -1)
        ed["acts"] = ed["acts"].reshape(-1).contiguous() if self.discrete else ed["acts"].contiguous()
        ed["dones"] = ed["dones"].bool().contiguous()
        gd = self._gen_dev._arrays
        B, mb = self.demo_batch_size, self.demo_minibatch_size
        dims = [lins[0].in_features] + [l.out_features for l in lins]
        gblk, fblk, n_params = self._C.disc_plan_sizes(dims, mb)
        assert n_params == n, (n_params, n)
        n_mb = B // mb
        z = lambda *sh, dt=th.float32: th.zeros(*sh, device=dev, dtype=dt)  # noqa: E731
        self._disc_ws = dict(X=z(2 * mb, dims[0]), partials=z(self._C.disc_partials_floats(mb, dims[0])), slab=z(n_mb * fblk * n),
                             stats_slab=z(n_mb * fblk * 8), grads=z(n), sums=z(2 * dims[0], dt=th.float64))
        self._disc_stats = z(max(1, self.n_disc_updates_per_round), 8)
        g = self._disc_opt.param_groups[0]
        d = dict(batch=B, minibatch=mb, W=[l.weight for l in lins], b=[l.bias for l in lins], hidden_act=int(hid),
                 rew_mean=norm.running_mean if norm is not None else None,
                 rew_var=norm.running_var if norm is not None else None,
                 rew_count=norm.count if norm is not None else None, rew_eps=float(norm.eps) if norm is not None else 1e-5,
                 obs_dim=self.D, act_width=self.A, use_state=int(base.use_state), use_action=int(base.use_action),
                 use_next_state=int(base.use_next_state), use_done=int(base.use_done), act_discrete=int(self.discrete),
                 e_obs=ed["obs"], e_next_obs=ed["next_obs"], e_acts=ed["acts"], e_dones=ed["dones"],
                 g_obs=gd["obs"], g_next_obs=gd["next_obs"], g_acts=gd["acts"], g_dones=gd["dones"],
                 pol_mean=self.pol_norm.running_mean if self.pol_norm is not None else None,
                 pol_var=self.pol_norm.running_var if self.pol_norm is not None else None,
                 pol_count=self.pol_norm.count if self.pol_norm is not None else None,
                 params=self._rflat.flat, exp_avg=self._r_m, exp_avg_sq=self._r_v,
                 beta1=float(g["betas"][0]), beta2=float(g["betas"][1]), eps=float(g["eps"]),
                 weight_decay=float(g.get("weight_decay", 0.0)), **self._disc_ws)
        self._disc_plan = self._C.DiscPlan(d)
        # Overlap (see train()): the round's discriminator updates run on a side stream
        # concurrently with its PPO update. They only read the expert set, the replay ring
        # and the reward net; their one write the PPO kernel also makes -- the policy
        # RunningNorm merge of the disc batch (GAIL's log-prob side effect) -- is recorded
        # per minibatch and applied in order after PPO, so the result is bitwise that of
        # the serial order.
        self._overlap_disc = os.environ.get("IMITATION_AMD_DISC_OVERLAP", "1") != "0"
        self._side_stream = shared_stream(dev, "engine_side") if self._overlap_disc else None
        self._pol_defer_buf = None
        if self._overlap_disc and self.pol_norm is not None and self._disc_plan.pol_cols > 0:
            self._ensure_pol_defer(max(1, self.n_disc_updates_per_round))
        self._disc_stats_host = th.zeros(max(1, self.n_disc_updates_per_round), 8, pin_memory=True)

    def _ensure_pol_defer(self, n_updates: int) -> None:
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

    @profiling.traced("disc/update")
    def _fused_disc_update(self, slot: int, defer_pol: bool = False) -> None:
        """One discriminator optimizer step (== AdversarialTrainer.train_disc) with no host sync.
        ``defer_pol``: record the policy-norm merges in slots ``slot * n_minibatches + k`` of
        the deferred-merge buffer instead of applying them (see :meth:`train`)."""
        if self._gen_dev.size() == 0:
            raise RuntimeError("No generator samples for training. Call `train_gen()` first.")
        opt = self._disc_opt
        self._adopt_disc_opt_state()
        g = opt.param_groups[0]
        t = float(opt.state[self._rflat.params[0]]["step"]) + 1.0
        beta1, beta2 = g["betas"]
        lr = float(g["lr"])
        step_size = lr / (1.0 - beta1**t)
        bc2_sqrt = (1.0 - beta2**t) ** 0.5
        B, mb = self.demo_batch_size, self.demo_minibatch_size
        e_idx = self._endless_expert_iterator.next_indices()
        g_idx = th.randint(0, self._gen_dev.size(), (B,), device=self._dev)
        merge_rew = self._rnorm is not None and self._rnorm.training
        merge_pol = self.pol_norm is not None and self.pol_norm.training
        plan = self._disc_plan
        stats_out = self._disc_stats[slot]
        base = slot * plan.n_minibatches if (defer_pol and merge_pol) else -1
        if pdist.world_size() == 1:
            plan.update(e_idx, g_idx, step_size, bc2_sqrt, merge_rew, merge_pol, stats_out, base)
        else:
            world = pdist.world_size()
            for k in range(B // mb):
                plan.gather(k, e_idx, g_idx)
                if merge_rew or merge_pol:
                    ds = base + k if base >= 0 else -1
                    if pdist.norm_sync_active():
                        plan.norm(1, 0, merge_rew, merge_pol)
                        pdist.allreduce_sum_(self._disc_ws["sums"])
                        plan.norm(2, 2 * mb * world, merge_rew, merge_pol, ds)
                    else:
                        plan.norm(0, 0, merge_rew, merge_pol, ds)
                plan.fwd_bwd(k)
            plan.adam(1, 0, 0.0, 1.0, stats_out)
            pdist.allreduce_grads_flat(self._disc_ws["grads"])
            plan.adam(0, 1, step_size, bc2_sqrt, None)
        for p in self._rflat.params:
            opt.state[p]["step"] += 1
        self._disc_step += 1

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
        if getattr(self, "_disc_graph", None) is None:
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
        if getattr(self, "_disc_stats_gen", None) is None or self._disc_stats_gen.shape[0] < n:
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
            pdist.check_comm("adversarial round")
            self._fail_if_nonfinite({f"update {i} sum {j}": float(v) for i in range(n) for j, v in enumerate(vals[i])},
                                    "discriminator")
            for i in range(n):
                with self.logger.accumulate_means("disc"):
                    self._record_disc(common.train_stats_from_sums(vals[i], rows), steps[i])
            if callback:
                callback(r)
            self.logger.dump(self._global_step)
        self.check_errors(blocking=True)

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
            self._disc_stats = th.zeros(n, 8, device=self._dev)
            self._disc_stats_host = th.zeros(n, 8, pin_memory=True)
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
            pdist.check_comm("GAIL round")
            if n:
                self._fail_if_nonfinite({f"update {i} sum {j}": float(v) for i in range(n) for j, v in enumerate(vals[i][:6])},
                                        "discriminator")
                for i in range(n):
                    with self.logger.accumulate_means("disc"):
                        self._record_disc(self._disc_stats_dict(vals[i]), steps[i])
            if callback:
                callback(r)
            self.logger.dump(self._global_step)
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
        """One GAIL round with its ``n`` discriminator updates on the side stream, concurrent
        with the PPO update (the round's rewards were already computed from the previous
        discriminator, so nothing PPO reads changes).

        ``ready``: the round's rollout was already enqueued (by the previous call) and this
        is its staging event. ``launch_next``: enqueue the next round's rollout behind this
        round's PPO + deferred merges BEFORE waiting for PPO on the host, so the GPU never
        idles while the host logs. Returns (disc steps, next round's staging event); the
        disc stats are in ``_disc_stats_host`` when this returns."""
        algo: PPO = self.gen_algo
        main = th.cuda.current_stream(self._dev)
        # AIRL (_disc_on_main): log pi needs the post-PPO policy, so the updates queue behind PPO
        # on the main stream -- the round is still pipelined: nothing waits on the host between
        # PPO, the updates and the next rollout
        side = main if getattr(self, "_disc_on_main", False) else self._side_stream
        pol_merge = self.pol_norm is not None and self.pol_norm.training
        defer = pol_merge and self._pol_defer_buf is not None
        if defer:
            self._ensure_pol_defer(n)
        # serial when the disc would write the norm PPO is using, or when both would issue
        # per-step collectives: the non-replicated DP PPO all-reduces every minibatch through
        # the same one-shot communicator as the disc, and two kernels in flight on it would
        # pair one rank's PPO gradients with another rank's disc sums
        serial = (pol_merge and not defer) or (pdist.world_size() > 1 and not self._dp_replicated)
        steps: List[int] = []
        nxt = None
        # AIRL split rounds: the updates' gathers + norm merges (the only part the next rollout's
        # step chain depends on, through the policy RunningNorm) are staged on the main stream;
        # the fwd/bwd + Adam applies run on the side stream concurrently with that chain, and
        # the rollout's reward pass waits for them
        # (single rank only; the policy-norm merges are on the main stream, ahead of the chain)
        split = getattr(self, "_disc_split", False) and n > 0
        with self.logger.accumulate_means("gen"):
            if algo._total_timesteps < algo.num_timesteps + self.T * self.N:
                algo._total_timesteps = algo.num_timesteps + self.T * self.N
            if ready is None:
                ready = self._launch_rollout()
            algo.num_timesteps += self.T * self.N
            self._ppo_update()
            ppo_done = self._ppo_done
            ready.synchronize()
            if split:
                return self._split_round(n, ppo_done, launch_next, steps)
            if serial:
                self._wait_ev(side, ppo_done)
            else:
                side.wait_event(ready)
            with th.cuda.stream(side):
                self._store_generator_samples()
                with networks.training(self.reward_train):
                    for i in range(n):
                        self._fused_disc_update(i, defer_pol=defer)
                        steps.append(self._disc_step)
                disc_dev = self._dev_event(side)
                self._disc_stats_host[:n].copy_(self._disc_stats[:n], non_blocking=True)
                disc_done = th.cuda.Event()
                disc_done.record(side)
            self._wait_ev(main, disc_dev)
            if defer:
                self._disc_plan.pol_norm_merge(n * self._disc_plan.n_minibatches)
            self._global_step += 1
            if launch_next:
                nxt = self._launch_rollout()
            ppo_done.synchronize()
            self._log_gen()
        disc_done.synchronize()
        return steps, nxt

    def _stage_during_ppo(self) -> bool:
        """Split-round staging on the side stream, concurrent with PPO. Under data parallelism
        only with the replicated PPO update, which issues no collective: the staging's normaliser
        all-reduces are then the only users of the communicator while they run.
        IMITATION_AMD_AIRL_EARLY_STAGE=0: stage behind PPO on the main stream."""
        return ((pdist.world_size() == 1 or self._dp_replicated) and self._host_staged
                and os.environ.get("IMITATION_AMD_AIRL_EARLY_STAGE", "1") != "0")

    def _split_round(self, n: int, ppo_done: th.cuda.Event, launch_next: bool,
                     steps: List[int]) -> Tuple[List[int], Optional[th.cuda.Event]]:
        """Rest of an AIRL split round after PPO (see _overlapped_round): stage the updates on
        the main stream, apply them on the side stream while the next rollout's step chain runs,
        then the rollout's reward pass behind the applies."""
        main = th.cuda.current_stream(self._dev)
        side = self._side_stream
        if self._stage_during_ppo():
            # replay store, gathers and base / potential merges on the side stream while PPO
            # runs (none of it touches the policy norm or the policy); then the policy-norm
            # merges, one launch, behind PPO on the main stream. The side stream is already
            # ordered after the rollout (_stage_rollout_to_host).
            with th.cuda.stream(side):
                self._store_generator_samples()
                with networks.training(self.reward_train):
                    scal = self._stage_disc_updates(n, defer_q=True)
                side_staged = self._dev_event(side)
            self._wait_ev(main, side_staged)
            self._merge_deferred_q(n)
            self._early_staged_rounds = getattr(self, "_early_staged_rounds", 0) + 1
        else:
            self._store_generator_samples()
            with networks.training(self.reward_train):
                scal = self._stage_disc_updates(n)
        staged = self._dev_event(main)
        # the next step chain is enqueued before the applies (host order only: it depends on
        # the staging, not on the applies), so a slow host never delays its start
        if launch_next:
            self._launch_chain()
        self._wait_ev(side, staged)
        with th.cuda.stream(side):
            self._apply_disc_updates(scal, steps)
            disc_dev = self._dev_event(side)
            self._disc_stats_host[:n].copy_(self._disc_stats[:n], non_blocking=True)
            disc_done = th.cuda.Event()
            disc_done.record(side)
        self._global_step += 1
        nxt = None
        if launch_next:
            self._wait_ev(main, disc_dev)
            reward = not self.debug_use_ground_truth
            self._launch_post(reward)
            if reward:
                self._post_rollout_rewards()
            nxt = self._stage_rollout_to_host()
        else:
            self._wait_ev(main, disc_dev)
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


class DeviceGAIL(DeviceEngineMixin, GAIL):
    """GAIL whose generator rounds run entirely on the GPU (see module docstring)."""

    _host_cls_name = "algorithms.adversarial.gail.GAIL"


def smoke_round(device) -> None:
    """Tiny end-to-end device round (used by ``__graft_entry__.smoke``)."""
    from imitation_amd.data import rollout as rollout_mod
    from imitation_amd.policies.base import FeedForward32Policy, NormalizeFeaturesExtractor
    from imitation_amd.util import logger as imit_logger
    from imitation_amd.util.util import make_vec_env

    rng = np.random.default_rng(0)
    venv = make_vec_env("seals/HalfCheetah-v1", rng=rng, n_envs=8)
    demo_env = make_vec_env("seals/HalfCheetah-v1", rng=np.random.default_rng(1), n_envs=4)
    demos = rollout_mod.flatten_trajectories(
        rollout_mod.generate_trajectories(None, demo_env, rollout_mod.make_min_timesteps(2048), rng=rng))
    gen = PPO(FeedForward32Policy, venv, n_steps=64, batch_size=64, n_epochs=2, device=device,
              policy_kwargs=dict(features_extractor_class=NormalizeFeaturesExtractor))
    rn = reward_nets.BasicRewardNet(venv.observation_space, venv.action_space, normalize_input_layer=networks.RunningNorm)
    tr = DeviceGAIL(demonstrations=demos, demo_batch_size=256, venv=venv, gen_algo=gen, reward_net=rn,
                    n_disc_updates_per_round=2, custom_logger=imit_logger.configure("/tmp/ia_smoke", format_strs=[]))
    tr.train(2 * 64 * 8)
    th.cuda.synchronize()
    assert all(th.isfinite(p).all() for p in gen.policy.parameters())
