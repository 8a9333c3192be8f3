"""The device PPO generator every device engine shares (:class:`DeviceGeneratorCore`; the table
in :mod:`imitation_amd.engine.gail` maps its kernels to the reference's host loop) and the
device replay of ``NormalizedRewardNet`` output normalisation (:class:`OutputNormMixin`).
The trainers' engines (:mod:`.adversarial` with :mod:`.gail` and :mod:`.airl`, :mod:`.preference`, :mod:`.rl`) build on
this module; it imports none of them."""

from __future__ import annotations

import contextlib
import os
import time
from typing import Any, Dict, List, Mapping, Optional, Sequence, Tuple

import numpy as np
import torch as th
from torch import nn

from imitation_amd import ops
from imitation_amd.data import types
from imitation_amd.envs import spaces
from imitation_amd.envs.vec_env import NativeVecEnv
from imitation_amd.ops import rl as rl_ops
from imitation_amd.ops.mlp import act_code
from imitation_amd.parallel import dist as pdist
from imitation_amd.rewards import reward_nets
from imitation_amd.rl.policies import ActorCriticPolicy
from imitation_amd.rl.ppo import PPO
from imitation_amd.util import networks
from imitation_amd.utils import profiling
from imitation_amd.utils.errflag import DeviceErrorFlag
from imitation_amd.utils.streams import shared_stream


def _unwrap_native(venv) -> Optional[NativeVecEnv]:
    e = venv
    while e is not None:
        if isinstance(e, NativeVecEnv):
            return e
        e = getattr(e, "venv", None)
    return None


def _mlp_layers(seq: nn.Sequential) -> Tuple[Optional[networks.BaseNorm], List[nn.Linear], int, int]:
    """(input norm, linears, hidden act code, out act code) of a build_mlp / trunk Sequential."""
    norm = None
    lins: List[nn.Linear] = []
    acts: List[int] = []
    for m in seq:
        if isinstance(m, networks.BaseNorm):
            norm = m
        elif isinstance(m, nn.Linear):
            lins.append(m)
            acts.append(0)
        elif isinstance(m, (nn.Flatten, networks.SqueezeLayer, nn.Dropout)):
            continue
        else:
            c = act_code(m)
            if c is None:
                raise ValueError(f"engine cannot fuse activation {m}")
            acts[-1] = c
    hidden = acts[0] if len(acts) > 1 else 0
    return norm, lins, hidden, acts[-1] if acts else 0


def _policy_nets(policy: ActorCriticPolicy):
    fe = policy.features_extractor
    norm = getattr(fe, "normalize", None)
    pi_trunk = list(policy.mlp_extractor.policy_net)
    vf_trunk = list(policy.mlp_extractor.value_net)

    def trunk(mods):
        lins, act = [], 0
        for m in mods:
            if isinstance(m, nn.Linear):
                lins.append(m)
            else:
                c = act_code(m)
                if c is None:
                    raise ValueError(f"engine cannot fuse activation {m}")
                act = c
        return lins, act

    pl, pa = trunk(pi_trunk)
    vl, va = trunk(vf_trunk)
    if pl and vl and pa != va:
        raise ValueError("actor and critic trunks must share the activation")
    return norm, pl + [policy.action_net], vl + [policy.value_net], pa or va


def supports_generator(venv, gen_algo) -> Tuple[bool, str]:
    """Env + PPO generator eligibility shared by the device GAIL / AIRL engines."""
    if not th.cuda.is_available():
        return False, "no GPU"
    nat = _unwrap_native(venv)
    if nat is None:
        return False, "env is not a native vector env"
    if nat._is_image:
        return False, "image observations"
    if not isinstance(gen_algo, PPO):
        return False, "generator is not PPO"
    pol = gen_algo.policy
    if type(pol).__name__.startswith("Homogenous") or not isinstance(pol, ActorCriticPolicy):
        return False, "policy is not a plain ActorCriticPolicy"
    if not pol.share_features_extractor:
        return False, "separate features extractors"
    try:
        norm, pl, vl, act = _policy_nets(pol)
    except ValueError as e:
        return False, str(e)
    dims = [pol.features_dim] + [l.out_features for l in pl]
    if max(dims) > 64 or len(pl) > 4 or len(vl) > 4:
        return False, "policy too wide / deep for the engine"
    if gen_algo.batch_size % 16 != 0:
        return False, "minibatch must be a multiple of 16"
    if (gen_algo.n_steps * gen_algo.n_envs) % gen_algo.batch_size != 0:
        return False, "rollout size not a multiple of the minibatch"
    if gen_algo.batch_size > 64 and not ppo_path(pol, nat, gen_algo.batch_size,
                                                 gen_algo.n_steps * gen_algo.n_envs).startswith("rc"):
        return False, "minibatch > 64 needs the register-chained PPO kernel, which rejects this policy"
    if gen_algo.clip_range_vf is not None or gen_algo.target_kl is not None:
        return False, "clip_range_vf / target_kl not supported by the engine"
    return True, ""


def _ppo_shape_args(pol: ActorCriticPolicy, nat, batch: int, rows: int, rc_gmax: int = 0) -> Dict[str, Any]:
    """The shape / planning part of the ``engine_ppo_*`` argument dict (what the host plan reads)."""
    norm, pl, vl, act = _policy_nets(pol)
    discrete = isinstance(nat.action_space, spaces.Discrete)
    D = int(np.prod(nat.observation_space.shape))
    A = int(nat.action_space.n) if discrete else int(np.prod(nat.action_space.shape))
    return dict(D=D, A=A, discrete=int(discrete), pi_dims=[D] + [l.out_features for l in pl],
                vf_dims=[D] + [l.out_features for l in vl], batch=int(batch), rows=int(rows),
                log_std_off=0 if (hasattr(pol, "log_std") and not discrete) else -1, rc_gmax=int(rc_gmax),
                hidden_act=int(act))


def ppo_path(pol: ActorCriticPolicy, nat, batch: int, rows: int, rc_gmax: int = 0) -> str:
    """Which PPO kernel the engine would run (``"rc:g<G>x<nch>x<cw>:kt<KT>"`` or ``"lds"``)."""
    return ops.native().engine_ppo_path(_ppo_shape_args(pol, nat, batch, rows, rc_gmax))


class _FlatParams:
    """Re-point a list of parameters at views of one flat fp32 device buffer."""

    def __init__(self, params: Sequence[nn.Parameter]):
        self.params = list(params)
        dev = self.params[0].device
        n = sum(p.numel() for p in self.params)
        self.flat = th.zeros(n, device=dev, dtype=th.float32)
        self.offsets = []
        off = 0
        for p in self.params:
            self.flat[off : off + p.numel()].copy_(p.detach().reshape(-1))
            self.offsets.append(off)
            p.data = self.flat[off : off + p.numel()].view_as(p)
            off += p.numel()
        self.n = n

    def offset(self, p: nn.Parameter) -> int:
        for q, o in zip(self.params, self.offsets):
            if q is p:
                return o
        raise KeyError("parameter not in flat buffer")


class DeviceGeneratorCore:
    """Device PPO generator: env state, flat policy parameters, the fused rollout kernel
    (policy + env + learned reward), GAE and the PPO update kernels, data-parallel plan.
    Shared by the adversarial engines (:class:`imitation_amd.engine.adversarial.DeviceEngineMixin`), the
    preference-comparison agent (:class:`imitation_amd.engine.preference.DeviceAgentTrainer`) and
    ``train_rl`` (:class:`imitation_amd.engine.rl.DevicePPO`).
    Subclasses set ``gen_algo``, ``_reward_net`` and ``debug_use_ground_truth`` and call
    :meth:`_init_generator`."""

    # ------------------------------------------------------------------ stream ordering
    def _dev_event(self, stream: Optional[th.cuda.Stream] = None):
        """An event recorded on ``stream`` (default: the current one) for GPU -> GPU ordering
        and host waits on completion: device-scope release (``_C.DeviceEvent``,
        csrc/bind/events.cpp), so the markers between the round's critical kernels do not write
        back the L2s. Pinned D2H copies the host reads keep torch (system-scope) events.
        IMITATION_AMD_DEVICE_EVENTS=0: torch events everywhere."""
        if os.environ.get("IMITATION_AMD_DEVICE_EVENTS", "1") != "0" and hasattr(self._C, "DeviceEvent"):
            ev = self._C.DeviceEvent(True)
            ev.record(stream.cuda_stream if stream is not None else None)
            return ev
        ev = th.cuda.Event()
        ev.record(stream)
        return ev

    @staticmethod
    def _wait_ev(stream: th.cuda.Stream, ev) -> None:
        """``stream`` waits for ``ev`` (a torch event or a ``_dev_event``)."""
        if isinstance(ev, th.cuda.Event):
            stream.wait_event(ev)
        else:
            ev.wait(stream.cuda_stream)

    def _init_generator(self, venv) -> None:
        self._native = _unwrap_native(venv)
        self._C = ops.native()
        self._dev = self.gen_algo.device
        self._setup_engine()
        self._setup_dp()

    # ------------------------------------------------------------------ setup
    def _setup_engine(self) -> None:
        dev = self._dev
        algo: PPO = self.gen_algo
        pol: ActorCriticPolicy = algo.policy
        nat = self._native
        self.N = nat.num_envs
        self.T = algo.n_steps
        self.D = int(np.prod(nat.observation_space.shape))
        self.discrete = isinstance(nat.action_space, spaces.Discrete)
        self.A = int(nat.action_space.n) if self.discrete else int(np.prod(nat.action_space.shape))
        # env state -> device
        obs0 = nat.reset()
        env = self._env_mirror(nat.get_state(), obs0)
        self.state, self.env_rng, self.elapsed = env["state"], env["rng"], env["elapsed"]
        self.ep_ret, self.cur_obs, self.cur_start = env["ep_ret"], env["cur_obs"], env["cur_start"]
        self.max_steps = int(nat.max_episode_steps)
        # policy parameters -> one flat buffer (module params become views)
        norm, pl, vl, hid = _policy_nets(pol)
        self.pol_norm = norm
        self.pi_layers, self.vf_layers, self.hidden_act = pl, vl, hid
        plist: List[nn.Parameter] = []
        for l in pl + vl:
            plist += [l.weight, l.bias]
        self.has_log_std = hasattr(pol, "log_std") and not self.discrete
        if self.has_log_std:
            plist.append(pol.log_std)
        self.flat = _FlatParams(plist)
        self.grads = th.zeros_like(self.flat.flat)
        self.exp_avg = th.zeros_like(self.flat.flat)
        self.exp_avg_sq = th.zeros_like(self.flat.flat)
        self.adam_step = th.zeros(1, device=dev)
        self.norm_count = norm.count.detach().float().reshape(1).clone() if norm is not None else None
        if self.discrete:
            self.act_low = self.act_high = None
        else:
            self.act_low = th.as_tensor(nat.action_space.low.reshape(-1), device=dev).float()
            self.act_high = th.as_tensor(nat.action_space.high.reshape(-1), device=dev).float()
        # rollout buffers [T, N, ...]
        T, N, D = self.T, self.N, self.D
        Aw = 1 if self.discrete else self.A
        z = lambda *s: th.zeros(*s, device=dev)
        self.buf = dict(obs_buf=z(T, N, D), act_raw=z(T, N, Aw), act_env=z(T, N, Aw), logp=z(T, N), values=z(T, N),
                        rewards=z(T, N), env_rew=z(T, N), starts=z(T, N), dones=z(T, N), trunc=z(T, N), boot=z(T, N),
                        next_obs=z(T, N, D), ep_ret_out=z(T, N), last_values=z(N))
        self._boot = self.buf["boot"]
        # PPO statistics sums (kernel output) followed by the GAE pass's [N][4] return /
        # advantage moments (train/explained_variance): ONE device buffer, one D2H copy per round
        self._log_dev = z(5 + 4 * N)
        self.stats = self._log_dev[:5]
        self._ev_mom = self._log_dev[5:].view(N, 4)
        self._seed = int(np.random.randint(0, 2**62)) ^ (pdist.rank() * 0x9E3779B97F4A7C15 & ((1 << 62) - 1))
        self._step0 = 0
        self._perm_round = 0
        self._ppo_err = DeviceErrorFlag(self._dev, "PPO update kernel")
        self._ppo_static = self._ppo_args_static()  # (sets _ppo_is_rc)
        self._ep_lens_running = np.zeros(self.N, dtype=np.int64)
        # per-round host state; the pinned buffers and streams are created at first use
        self._ppo_log_host = self._ppo_std_host = self._log_stream = self._ppo_log_event = None  # _stage_ppo_logs
        self._ppo_done = self._last_ppo_info = self._last_clip_range = self._last_lr = None  # _ppo_update
        self._host_stage, self._host_staged = None, False  # _stage_rollout_to_host
        self._side_stream = None  # (engine/adversarial.py _setup_fused_disc)
        self._fps_mark = (None, None)

    def _env_mirror(self, st: Mapping[str, np.ndarray], obs0) -> Dict[str, th.Tensor]:
        """Device tensors of a native env block just reset (``get_state()``, reset observations),
        keyed as the rollout chain kernel names them."""
        dev = self._dev
        n = len(st["elapsed"])
        return dict(state=th.as_tensor(st["state"], device=dev).float().contiguous(),
                    rng=th.as_tensor(st["rng"].astype(np.int64), device=dev).contiguous(),
                    elapsed=th.as_tensor(st["elapsed"].astype(np.int32), device=dev).contiguous(),
                    ep_ret=th.zeros(n, device=dev),
                    cur_obs=th.as_tensor(np.asarray(obs0, np.float32), device=dev).reshape(n, self.D).contiguous(),
                    cur_start=th.ones(n, device=dev))

    def _env_tensors(self) -> Dict[str, th.Tensor]:
        """The training envs' mirror, keyed like :meth:`_env_mirror`."""
        return dict(state=self.state, rng=self.env_rng, elapsed=self.elapsed, ep_ret=self.ep_ret,
                    cur_obs=self.cur_obs, cur_start=self.cur_start)

    def _wave_mlp(self, lins: Sequence[nn.Linear], hidden_act: int, out_act: int, norm=None) -> Dict[str, Any]:
        d: Dict[str, Any] = dict(W=[l.weight.detach() for l in lins], b=[l.bias.detach() for l in lins],
                                 hidden_act=int(hidden_act), out_act=int(out_act))
        if norm is not None:
            d.update(norm_mean=norm.running_mean.detach().float().contiguous(),
                     norm_var=norm.running_var.detach().float().contiguous(), norm_eps=float(norm.eps))
        return d

    def _reward_spec(self) -> Dict[str, Any]:
        _, base = _split(self._reward_net)
        rnorm, rl, rh, ro = _mlp_layers(base.mlp)
        return dict(rew=self._wave_mlp(rl, rh, ro, rnorm), use_state=int(base.use_state), use_action=int(base.use_action),
                    use_next_state=int(base.use_next_state), use_done=int(base.use_done), rew_transform=1)

    def _post_rollout_rewards(self) -> None:
        """Hook: rewrite ``buf["rewards"]`` after the rollout kernel (AIRL output normalisation)."""

    def _ppo_args_static(self) -> Dict[str, Any]:
        algo: PPO = self.gen_algo
        fp = self.flat
        d = _ppo_shape_args(algo.policy, self._native, algo.batch_size, self.T * self.N)
        d.update(pi_w_off=[fp.offset(l.weight) for l in self.pi_layers], pi_b_off=[fp.offset(l.bias) for l in self.pi_layers],
                 vf_w_off=[fp.offset(l.weight) for l in self.vf_layers], vf_b_off=[fp.offset(l.bias) for l in self.vf_layers],
                 log_std_off=fp.offset(self.gen_algo.policy.log_std) if self.has_log_std else -1,
                 params=fp.flat, grads=self.grads, exp_avg=self.exp_avg, exp_avg_sq=self.exp_avg_sq, n_params=fp.n,
                 has_norm=int(self.pol_norm is not None), n_epochs=int(algo.n_epochs),
                 ent_coef=float(algo.ent_coef), vf_coef=float(algo.vf_coef), max_grad_norm=float(algo.max_grad_norm),
                 normalize_advantage=int(algo.normalize_advantage), adam_step=self.adam_step, stats=self.stats,
                 err=self._ppo_err.word,
                 # fail-fast knobs of the cooperating-workgroup kernel (tests force a timeout)
                 spin_limit=0, debug_stall=0,  # (tests set these two in _ppo_static)
                 # one row group without cycle counters runs the lean kernel instance of its shape
                 # (csrc/kernels/ppo_rc_instances.h); 0 keeps the full one (bitwise the same update)
                 rc_lean=1)
        opt = algo.policy.optimizer
        g = opt.param_groups[0]
        d.update(beta1=float(g.get("betas", (0.9, 0.999))[0]), beta2=float(g.get("betas", (0.9, 0.999))[1]),
                 adam_eps=float(g.get("eps", 1e-8)))
        if self.pol_norm is not None:
            d.update(norm_mean=self.pol_norm.running_mean, norm_var=self.pol_norm.running_var, norm_count=self.norm_count,
                     norm_eps=float(self.pol_norm.eps))
        self._ppo_is_rc = self._C.engine_ppo_path(d).startswith("rc")
        if not self._ppo_is_rc:
            lds = self._C.engine_ppo_lds(d) if d["batch"] <= 64 else 1 << 30
            if lds > 150 * 1024:
                raise ValueError(f"PPO engine needs {lds} B of LDS (> 150 KiB)")
        return d

    # ------------------------------------------------------------------ one generator round
    _CHAIN_OUT = ("obs_buf", "act_raw", "act_env", "env_rew", "starts", "dones", "trunc", "next_obs", "ep_ret_out")

    @profiling.traced("rollout/chain")
    def _launch_chain(self, explore_mode: Optional[th.Tensor] = None) -> None:
        """The serial part of a rollout (rollout.hip): T steps of actor sampling + env
        physics per env, nothing else on the step chain."""
        args = self._chain_args(self._env_tensors(), self.T, self.N, int(self._seed), int(self._step0), explore_mode)
        args.update({k: self.buf[k] for k in self._CHAIN_OUT})
        self._C.engine_rollout(args)
        self._step0 += self.T

    def _chain_args(self, block: Mapping[str, th.Tensor], T: int, N: int, seed: int, step0: int,
                    explore_mode: Optional[th.Tensor] = None, deterministic: bool = False) -> Dict[str, Any]:
        """``engine_rollout`` arguments for the env ``block`` (:meth:`_env_mirror` keys) under the
        current policy, without the output buffers."""
        return dict(block, env=self._native.env_id, max_steps=self.max_steps, T=T, N=N, seed=seed, step0=step0,
                    pi=self._wave_mlp(self.pi_layers, self.hidden_act, 0, self.pol_norm),
                    log_std=self.gen_algo.policy.log_std.detach() if self.has_log_std else None,
                    act_low=self.act_low, act_high=self.act_high, n_actions=self.A if self.discrete else 0,
                    explore_mode=explore_mode, deterministic=int(deterministic))

    _POST_BUFS = ("obs_buf", "act_raw", "act_env", "next_obs", "trunc", "env_rew", "values", "logp", "boot",
                  "rewards", "last_values")

    def _post_args(self, bufs: Mapping[str, th.Tensor], cur_obs: th.Tensor, T: int, N: int, dones: th.Tensor,
                   reward: bool) -> Dict[str, Any]:
        """``engine_rollout_post`` arguments over the rollout buffers ``bufs`` of a ``[T, N]`` block
        whose envs now stand at ``cur_obs`` (with the reward spec when ``reward``)."""
        algo: PPO = self.gen_algo
        d = dict(T=T, N=N, D=self.D, A=1 if self.discrete else self.A, n_actions=self.A if self.discrete else 0,
                 gamma=float(algo.gamma), cur_obs=cur_obs, dones=dones,
                 pi=self._wave_mlp(self.pi_layers, self.hidden_act, 0, self.pol_norm),
                 vf=self._wave_mlp(self.vf_layers, self.hidden_act, 0, self.pol_norm),
                 log_std=algo.policy.log_std.detach() if self.has_log_std else None, rew_enabled=int(reward))
        d.update({k: bufs[k] for k in self._POST_BUFS})
        if reward:
            d.update(self._reward_spec())
        return d

    @profiling.traced("rollout/reward_pass")
    def _launch_post(self, reward: bool) -> None:
        """The parallel part (engine.hip): V(s), log-probs, TimeLimit bootstrap and the learned
        reward of all T x N transitions, V of the final observations."""
        d = self._post_args(self.buf, self.cur_obs, self.T, self.N, self.buf["dones"], reward)
        if reward:
            d.update(self._rollout_extra_bufs())
        self._C.engine_rollout_post(d)

    def _rollout(self) -> None:
        """One training rollout: chain -> parallel pass (-> AIRL output normalisation). The
        learned reward does not feed back into the dynamics, so it leaves the step chain."""
        self._launch_chain()
        reward = not self.debug_use_ground_truth
        self._launch_post(reward)
        if reward:
            self._post_rollout_rewards()

    def _rollout_extra_bufs(self) -> Dict[str, Any]:
        return {}

    @profiling.traced("ppo/update")
    def _ppo_update(self) -> None:
        algo: PPO = self.gen_algo
        rows = self.T * self.N
        world = pdist.world_size()
        # single-rank fast path: the kernel reads / writes the module's int32 count itself and
        # its prep launch zeroes the stats (three small launches fewer between the rollout
        # and the update)
        direct = (world == 1 and self._ppo_is_rc
                  and (self.pol_norm is None or self.pol_norm.count.dtype == th.int32))
        if self.pol_norm is not None and not direct:
            # the policy normaliser may also have been updated outside the engine (the
            # discriminator's log-prob pass runs the policy in training mode, as the
            # reference does): the kernel continues from the module's own count
            self.norm_count.copy_(self.pol_norm.count.reshape(1))
        algo._update_current_progress_remaining(algo.num_timesteps, algo._total_timesteps or algo.num_timesteps)
        lr = float(algo.lr_schedule(algo._current_progress_remaining))
        clip = float(algo.clip_range(algo._current_progress_remaining))
        adv, ret = rl_ops.gae(self.buf["rewards"], self.buf["values"], self.buf["starts"], self.buf["last_values"],
                              self.cur_start, float(algo.gamma), float(algo.gae_lambda), moments=self._ev_mom)
        self._last_clip_range, self._last_lr = clip, lr
        obs = self.buf["obs_buf"].reshape(rows, self.D)
        acts = self.buf["act_raw"].reshape(rows, -1)
        old_logp = self.buf["logp"].reshape(rows)
        adv = adv.reshape(rows).contiguous()
        ret = ret.reshape(rows).contiguous()
        d = dict(self._ppo_static)
        d.update(clip_range=clip, lr=lr)
        if direct:
            d.update(zero_stats=1, norm_count_i=self.pol_norm.count if self.pol_norm is not None else None)
        else:
            self.stats.zero_()
        if world == 1:
            perm = self._epoch_perms(rows, self._seed)
            d.update(obs=obs, acts=acts, old_logp=old_logp, adv=adv, returns=ret, perm=perm, mode=0)
            self._C.engine_ppo_update(d)
        elif self._dp_replicated:
            self._ppo_update_replicated(d, obs, acts, old_logp, adv, ret)
        else:
            perm = self._epoch_perms(rows, self._seed)
            d.update(obs=obs, acts=acts, old_logp=old_logp, adv=adv, returns=ret, perm=perm)
            n_mb = rows // algo.batch_size
            B = algo.batch_size
            for it in range(algo.n_epochs * n_mb):
                e, mb = divmod(it, n_mb)
                if self.pol_norm is not None:
                    idx = perm[e, mb * B : (mb + 1) * B].long()
                    self._dp_norm_update(obs.index_select(0, idx))
                d["mode"] = 1
                d["mb_index"] = it
                self._C.engine_ppo_update(d)
                pdist.allreduce_grads_flat(self.grads)
                d["mode"] = 2
                self._C.engine_ppo_update(d)
        if self.pol_norm is not None and not direct:
            self.pol_norm.count.copy_(self.norm_count.to(self.pol_norm.count.dtype).reshape(()))
        # one marker behind the update: the round's host wait and the log copies' stream order
        self._ppo_done = self._dev_event()
        algo._n_updates += algo.n_epochs
        self._last_ppo_info = (rows, algo.n_epochs * (rows // algo.batch_size))
        self._stage_ppo_logs()
        # reads the error word of an EARLIER update (non-blocking; its copy on the log stream,
        # off the update -> next chain path); train() ends blocking
        self._ppo_err.check("PPO update", stream=self._log_stream)

    def _stage_ppo_logs(self) -> None:
        """Async D2H copy (stream order: right behind the update) of the update's statistics, the
        explained-variance moments and log_std into pinned memory; :meth:`_ppo_log_values` reads
        them after the copy event -- no blocking read of device tensors at logging time (the next
        round may already be enqueued behind the update)."""
        if self._ppo_log_host is None:
            self._ppo_log_host = th.zeros(self._log_dev.numel(), pin_memory=True)
            self._ppo_std_host = th.zeros(self.A, pin_memory=True) if self.has_log_std else None
        # on a stream of their own: the copies stay off the update -> next rollout chain, and off
        # the side stream the discriminator updates (enqueued after this) run on concurrently
        # with the update. The next round's update, which rewrites these buffers, is enqueued
        # only after the host has waited for this event.
        if self._log_stream is None:
            self._log_stream = shared_stream(self._dev, "engine_log")
        self._wait_ev(self._log_stream, self._ppo_done)  # (_ppo_update has just recorded it)
        with th.cuda.stream(self._log_stream):
            self._ppo_log_host.copy_(self._log_dev, non_blocking=True)
            if self._ppo_std_host is not None:
                self._ppo_std_host.copy_(self.gen_algo.policy.log_std.detach().reshape(-1), non_blocking=True)
            self._ppo_log_event = th.cuda.Event()
            self._ppo_log_event.record()

    def _record_round_metrics(self) -> None:
        """The host PPO's per-round records (``rl/ppo.py`` ``train`` + ``rl/base.py``
        ``_dump_logs``) for one device round."""
        algo = self.gen_algo
        lg = self.logger
        vals = self._ppo_log_values()
        self._fail_if_nonfinite({k: v for k, v in vals.items() if k != "train/explained_variance"}, "PPO update")
        for k, v in vals.items():
            lg.record(k, v)
        lg.record("train/n_updates", algo._n_updates, exclude="tensorboard")
        now = time.perf_counter()
        t_prev, n_prev = self._fps_mark
        if t_prev is not None and now > t_prev and algo.num_timesteps > n_prev:
            dt = now - t_prev
            lg.record("time/fps", int((algo.num_timesteps - n_prev) / dt))
            lg.record("time/time_elapsed", int(dt), exclude="tensorboard")
        self._fps_mark = (now, algo.num_timesteps)
        lg.record("time/iterations", 1, exclude="tensorboard")
        lg.record("time/total_timesteps", algo.num_timesteps, exclude="tensorboard")
        if algo.ep_info_buffer:
            lg.record("rollout/ep_rew_mean", float(np.mean([e["r"] for e in algo.ep_info_buffer])))
            lg.record("rollout/ep_len_mean", float(np.mean([e["l"] for e in algo.ep_info_buffer])))

    def _fail_if_nonfinite(self, values: Mapping[str, float], what: str) -> None:
        """Fail fast (the reference raises on broken invariants, e.g.
        ``algorithms/base.py:77-110``): the round's statistics are already on the host, so this
        costs no device sync. A NaN / Inf loss means the weights it came from are poisoned."""
        bad = [k for k, v in values.items() if not np.isfinite(v)]
        if bad:
            from imitation_amd.utils.watchdog import NonFiniteError

            rnd = getattr(self, "_global_step", None)
            raise NonFiniteError(f"non-finite {what} statistics{'' if rnd is None else f' in round {rnd}'}: "
                                 f"{', '.join(bad)}")

    def _ppo_log_values(self) -> Dict[str, float]:
        """SB3 ``PPO.train`` metrics of the latest update (reference keys, ``rl/ppo.py``): means of
        the per-minibatch sums, ``train/loss`` from those means (SB3 logs the last minibatch's),
        explained variance of the round's values vs GAE returns, std of the Gaussian head."""
        self._ppo_log_event.synchronize()
        algo: PPO = self.gen_algo
        h = self._ppo_log_host.numpy()
        rows, n_mb = self._last_ppo_info
        s = h[:5] / max(1, n_mb)
        out = {"train/entropy_loss": float(s[0]), "train/policy_gradient_loss": float(s[1]),
               "train/value_loss": float(s[2]), "train/clip_fraction": float(s[3]), "train/approx_kl": float(s[4]),
               "train/loss": float(s[1] + algo.ent_coef * s[0] + algo.vf_coef * s[2]),
               "train/explained_variance": rl_ops.explained_variance_from_moments(h[5:], rows),
               "train/clip_range": float(self._last_clip_range), "train/learning_rate": float(self._last_lr)}
        if self._ppo_std_host is not None:
            out["train/std"] = float(np.exp(self._ppo_std_host.numpy()).mean())
        return out

    def check_errors(self, blocking: bool = False) -> None:
        """Raise if a cooperating PPO workgroup timed out in any update so far."""
        self._ppo_err.check("PPO update", blocking=blocking)

    def _setup_dp(self) -> None:
        """Data-parallel PPO plan. With the register-chained kernel available for the global
        minibatch (world x batch rows), every rank all-gathers the round's rollout rows
        (ONE collective of rows x (D + A + 3) floats) and runs the identical, deterministic
        update over the global batch -- exactly synchronous DP (averaged minibatch gradients,
        global advantage / normaliser statistics), with no per-minibatch collective. The
        minibatch permutation comes from a generator seeded identically on every rank.
        Otherwise the per-minibatch grad/all-reduce/apply kernels are used."""
        world = pdist.world_size()
        self._dp_replicated = False
        if world <= 1:
            return
        algo: PPO = self.gen_algo
        rows = self.T * self.N
        path = ppo_path(algo.policy, self._native, algo.batch_size * world, rows * world)
        self._dp_replicated = path.startswith("rc")
        self._dp_perm_seed = int(pdist.broadcast_object(int(np.random.randint(0, 2**62))))
        Aw = 1 if self.discrete else self.A
        self._dp_cols = (self.D, Aw)
        self._dp_pack = th.zeros(rows, self.D + Aw + 3, device=self._dev)
        self._dp_global = th.zeros(world * rows, self.D + Aw + 3, device=self._dev)

    def _ppo_update_replicated(self, d: Dict[str, Any], obs, acts, old_logp, adv, ret) -> None:
        algo: PPO = self.gen_algo
        world = pdist.world_size()
        rows = obs.shape[0]
        D, Aw = self._dp_cols
        pk = self._dp_pack
        pk[:, :D] = obs
        pk[:, D : D + Aw] = acts
        pk[:, D + Aw] = old_logp
        pk[:, D + Aw + 1] = adv
        pk[:, D + Aw + 2] = ret
        pdist.all_gather_flat(self._dp_global, pk)
        gl = self._dp_global
        rows_g = world * rows
        perm = self._epoch_perms(rows_g, self._dp_perm_seed)
        d.update(obs=gl[:, :D].contiguous(), acts=gl[:, D : D + Aw].contiguous(),
                 old_logp=gl[:, D + Aw].contiguous(), adv=gl[:, D + Aw + 1].contiguous(),
                 returns=gl[:, D + Aw + 2].contiguous(), perm=perm, rows=rows_g, batch=algo.batch_size * world,
                 mode=0, allow_rc=1)
        self._C.engine_ppo_update(d)
        # stats are sums over the global minibatches; every rank holds the same model

    def _epoch_perms(self, rows: int, base_seed: int) -> th.Tensor:
        """``[n_epochs, rows]`` int32 minibatch orders of this update: one ``perm_feistel``
        launch keyed by (base seed, update counter) -- replicas that share the base seed
        (replicated DP) draw identical orders, and the counter is checkpointed."""
        self._perm_round += 1
        key = (int(base_seed) * 0x9E3779B97F4A7C15 + self._perm_round) & ((1 << 64) - 1)
        return rl_ops.random_permutations(self.gen_algo.n_epochs, rows, key, self._dev)

    def _dp_norm_update(self, batch: th.Tensor) -> None:
        """RunningNorm.update_stats with all-reduced moments (the kernel is told not to update)."""
        norm = self.pol_norm
        mean, var, cnt = pdist.allreduce_moments(batch)
        c0 = self.norm_count
        tot = c0 + cnt
        delta = mean - norm.running_mean
        norm.running_mean.add_(delta * cnt / tot)
        rv = norm.running_var * c0 + var * cnt + delta.square() * c0 * cnt / tot
        norm.running_var.copy_(rv / tot)
        self.norm_count.add_(cnt)

    def _eval_block(self, n: int, seed: int, deterministic: bool, reward: bool):
        """A fresh block of ``n`` native envs (reset from ``seed``) and the scratch buffers of one
        ``max_episode_steps`` launch of the rollout chain (+ the reward pass when ``reward``)."""
        ev = NativeVecEnv(self._native.env_id, n, seed=int(seed), max_episode_steps=self.max_steps)
        obs0 = ev.reset()
        T = self.max_steps  # every env finishes >= 1 episode per launch (TimeLimit)
        Aw = 1 if self.discrete else self.A
        z = lambda *s: th.zeros(*s, device=self._dev)  # noqa: E731
        bufs = dict(obs_buf=z(T, n, self.D), act_raw=z(T, n, Aw), act_env=z(T, n, Aw), env_rew=z(T, n),
                    starts=z(T, n), trunc=z(T, n), next_obs=z(T, n, self.D))
        if reward:
            bufs.update(values=z(T, n), logp=z(T, n), boot=z(T, n), rewards=z(T, n), last_values=z(n))
        # (callers set step0 per launch)
        args = self._chain_args(self._env_mirror(ev.get_state(), obs0), T, n,
                                int(seed) * 0x2545F4914F6CDD1D & ((1 << 62) - 1), 0, deterministic=deterministic)
        return T, bufs, args

    def _eval_learned_reward(self, T: int, n: int, bufs: Dict[str, th.Tensor], args: Dict[str, Any],
                             dones: th.Tensor, out: th.Tensor) -> None:
        """The learned reward of one eval launch (the reward pass of training rollouts, written
        without the TimeLimit bootstrap) into ``out`` [T, n]."""
        # (no _rollout_extra_bufs: see _eval_supports_learned_reward)
        self._C.engine_rollout_post(self._post_args(bufs, args["cur_obs"], T, n, dones, reward=True))
        out.copy_(bufs["rewards"] - bufs["boot"])

    def _eval_supports_learned_reward(self) -> bool:
        """AIRL's output normalisation runs in a separate pass over the training buffers; its
        evaluation-time rewards come from the host path."""
        out_norm = getattr(self, "_output_norm", None)
        return out_norm is None or out_norm() is None

    @profiling.traced("eval/device")
    def device_evaluate(self, n_eval_episodes: int = 10, deterministic: bool = True, n_envs: Optional[int] = None,
                        seed: int = 0) -> Tuple[List[float], List[int]]:
        """``evaluate_policy(policy, venv, n_eval_episodes, deterministic, return_episode_rewards=True)``
        on the GPU (reference ``stable_baselines3.common.evaluation.evaluate_policy``, the metric
        of ``scripts/ingredients/policy_evaluation.py``): a separate block of ``n_envs`` native
        envs (default: the training count) reset from ``seed`` and stepped by the rollout chain
        kernel with the current policy (mean / argmax actions when ``deterministic``), one
        ``max_episode_steps`` launch per episode slot -- no host round trip per step. Env ``i``
        contributes its first ``(n_eval_episodes + i) // n_envs`` episodes, as SB3 counts them;
        returns (episode returns, episode lengths) in completion order. The training envs, the
        policy and every normaliser are untouched."""
        n = int(n_envs or self.N)
        targets = np.array([(n_eval_episodes + i) // n for i in range(n)], dtype=np.int64)
        n_chunks = int(targets.max(initial=0))
        if n_chunks == 0:
            return [], []
        T, bufs, args = self._eval_block(n, seed, deterministic, reward=False)
        dones = th.zeros(n_chunks, T, n, device=self._dev)
        rets = th.zeros(n_chunks, T, n, device=self._dev)
        for c in range(n_chunks):
            args.update(bufs, step0=c * T, dones=dones[c], ep_ret_out=rets[c])
            self._C.engine_rollout(args)
        d = dones.reshape(n_chunks * T, n).cpu().numpy() > 0.5
        r = rets.reshape(n_chunks * T, n).cpu().numpy()
        ts, es = np.nonzero(d)  # row-major: completion step, then env
        ep_rewards: List[float] = []
        ep_lengths: List[int] = []
        last = np.full(n, -1, dtype=np.int64)
        count = np.zeros(n, dtype=np.int64)
        for t, e in zip(ts.tolist(), es.tolist()):
            length = t - last[e]
            last[e] = t
            if count[e] < targets[e]:
                ep_rewards.append(float(r[t, e]))
                ep_lengths.append(int(length))
                count[e] += 1
        return ep_rewards, ep_lengths

    def device_demonstrations(self, min_timesteps: int, deterministic: bool = False, seed: int = 0,
                              n_envs: Optional[int] = None) -> types.Transitions:
        """Rollouts of the current policy as flat demonstration transitions (``rollout.rollout`` +
        ``flatten_trajectories`` of whole episodes, the way the reference's experts are rolled out
        for the benchmarks) from a fresh env block on the GPU: launches of ``max_episode_steps``
        until ``min_timesteps`` transitions of finished episodes are collected; episodes in
        completion order (per launch: by env), each in time order; ``dones`` marks true
        terminations only (a TimeLimit cut is not terminal)."""
        n = int(n_envs or self.N)
        T, bufs, args = self._eval_block(n, seed, deterministic, reward=False)
        parts: Dict[str, List[np.ndarray]] = {k: [] for k in ("obs", "acts", "next_obs", "dones")}
        carry = [dict(obs=[], acts=[], next_obs=[]) for _ in range(n)]  # episodes spanning launches
        got, c = 0, 0
        while got < min_timesteps:
            dones = th.zeros(T, n, device=self._dev)
            args.update(bufs, step0=c * T, dones=dones, ep_ret_out=th.zeros(T, n, device=self._dev))
            self._C.engine_rollout(args)
            c += 1
            d = dones.cpu().numpy() > 0.5
            obs, nxt = bufs["obs_buf"].cpu().numpy(), bufs["next_obs"].cpu().numpy()
            acts = bufs["act_env"].cpu().numpy()
            trunc = bufs["trunc"].cpu().numpy() > 0.5
            for e in range(n):
                cur = carry[e]
                t0 = 0
                for t in np.flatnonzero(d[:, e]).tolist() + [None]:
                    t1 = T if t is None else t + 1
                    cur["obs"].append(obs[t0:t1, e])
                    cur["acts"].append(acts[t0:t1, e])
                    cur["next_obs"].append(nxt[t0:t1, e])
                    if t is not None:
                        length = sum(len(x) for x in cur["acts"])
                        for k in ("obs", "acts", "next_obs"):
                            parts[k].append(np.concatenate(cur[k]))
                            cur[k] = []
                        dn = np.zeros(length, dtype=bool)
                        dn[-1] = not trunc[t, e]
                        parts["dones"].append(dn)
                        got += length
                    t0 = t1
        acts = np.concatenate(parts["acts"])
        if self.discrete:
            acts = acts.reshape(-1).astype(np.int64)
        return types.Transitions(obs=np.concatenate(parts["obs"]).astype(np.float32), acts=acts,
                                 next_obs=np.concatenate(parts["next_obs"]).astype(np.float32),
                                 dones=np.concatenate(parts["dones"]), infos=np.array([{}] * len(acts)))

    @profiling.traced("eval/device_stats")
    def device_rollout_stats(self, n_episodes: int, deterministic: bool = False, seed: Optional[int] = None,
                             n_envs: Optional[int] = None) -> Optional[Dict[str, float]]:
        """``rollout_stats(generate_trajectories(policy, venv_train, make_min_episodes(n)))`` -- the
        CLI's final ``imit_stats`` (reference ``scripts/ingredients/policy_evaluation.py``) -- on the
        GPU: stochastic actions by default (``generate_trajectories``' default), the same
        unbiased stopping (once >= ``n`` episodes are done, every env finishes its episode in
        flight and stops), ``return_*`` from the learned reward the training rollouts see and
        ``monitor_return_*`` / ``len_*`` from the env. A fresh env block reset from ``seed``
        (default: derived from the engine seed); the training state is untouched. Returns None
        where the learned reward is not available on this path (AIRL with output normalisation)."""
        if not self._eval_supports_learned_reward():
            return None
        n = int(n_envs or self.N)
        seed = int(self._seed % (1 << 31)) + 7 if seed is None else int(seed)
        T, bufs, args = self._eval_block(n, seed, deterministic, reward=not self.debug_use_ground_truth)
        dl, rl, wl = [], [], []
        count = 0
        c = 0
        finishing = False
        while True:  # launches until >= n episodes, then one more so every in-flight episode ends
            dones, rets = th.zeros(T, n, device=self._dev), th.zeros(T, n, device=self._dev)
            args.update(bufs, step0=c * T, dones=dones, ep_ret_out=rets)
            self._C.engine_rollout(args)
            if self.debug_use_ground_truth:
                w = bufs["env_rew"].clone()
            else:
                w = th.zeros(T, n, device=self._dev)
                self._eval_learned_reward(T, n, bufs, args, dones, w)
            dl.append(dones)
            rl.append(rets)
            wl.append(w)
            c += 1
            if finishing:
                break
            count += int(dones.sum().item())
            finishing = count >= n_episodes
        d = th.cat(dl).cpu().numpy() > 0.5
        r = th.cat(rl).cpu().numpy()
        wr = th.cat(wl).double().cpu().numpy()
        cs = np.cumsum(wr, axis=0)
        active = np.ones(n, dtype=bool)
        start = np.zeros(n, dtype=np.int64)
        rets, lens, mon = [], [], []
        for t in range(d.shape[0]):
            fin = np.flatnonzero(d[t] & active)
            for e in fin.tolist():
                ln = t - start[e] + 1
                rets.append(float(cs[t, e] - (cs[start[e] - 1, e] if start[e] > 0 else 0.0)))
                lens.append(int(ln))
                mon.append(float(r[t, e]))
            for e in np.flatnonzero(d[t]).tolist():
                start[e] = t + 1
            if len(rets) >= n_episodes:
                active &= ~d[t]
            if not active.any():
                break
        out: Dict[str, float] = {"n_traj": len(rets)}
        for name, vals in (("return", np.asarray(rets)), ("len", np.asarray(lens)), ("monitor_return", np.asarray(mon))):
            for stat in ("min", "mean", "std", "max"):
                out[f"{name}_{stat}"] = getattr(np, stat)(vals).item()
        out["monitor_return_len"] = len(mon)
        return out

    def sync_env_to_host(self) -> None:
        """Copy the device env state back into the native host env (e.g. before host-side evaluation)."""
        self._native.set_state({"state": self.state.cpu().numpy(), "rng": self.env_rng.cpu().numpy(),
                                "elapsed": self.elapsed.cpu().numpy().astype(np.int64)})

    def _stage_rollout_to_host(self):
        """Async D2H copy of (dones, episode returns) into pinned buffers; returns the event
        that marks them ready."""
        wrapped = not self.debug_use_ground_truth
        if self._host_stage is None:
            self._host_stage = th.empty(4 if wrapped else 2, self.T, self.N, pin_memory=True)
        # on the side stream: the copies stay off the rollout -> GAE -> PPO chain (the host
        # waits for this event before the next rollout can overwrite the buffers)
        side = self._side_stream
        if side is not None:
            self._wait_ev(side, self._dev_event())
        with th.cuda.stream(side) if side is not None else contextlib.nullcontext():
            self._host_stage[0].copy_(self.buf["dones"], non_blocking=True)
            self._host_stage[1].copy_(self.buf["ep_ret_out"], non_blocking=True)
            if wrapped:  # learned reward = rewards - TimeLimit bootstrap (RewardVecEnvWrapper's rews)
                self._host_stage[2].copy_(self.buf["rewards"], non_blocking=True)
                self._host_stage[3].copy_(self._boot, non_blocking=True)
            ev = th.cuda.Event()
            ev.record()
        self._host_staged = True
        return ev

    # ------------------------------------------------------------------ checkpoint / resume
    _ENGINE_TENSORS: Tuple[str, ...] = ("exp_avg", "exp_avg_sq", "adam_step", "state", "env_rng", "elapsed", "ep_ret",
                                        "cur_obs", "cur_start")

    def _core_engine_state(self) -> Dict[str, Any]:
        """The part of every engine's ``engine_state`` (parameters live in the policy modules)."""
        st: Dict[str, Any] = {k: getattr(self, k).detach().cpu().clone() for k in self._ENGINE_TENSORS}
        if self.norm_count is not None:
            if self.pol_norm is not None:  # (the single-rank update keeps the module's count only)
                self.norm_count.copy_(self.pol_norm.count.reshape(1))
            st["norm_count"] = self.norm_count.cpu().clone()
        st.update(step0=int(self._step0), seed=int(self._seed), perm_round=int(self._perm_round))
        return st

    def _load_core_engine_state(self, st: Mapping[str, Any]) -> None:
        with th.no_grad():
            for k in self._ENGINE_TENSORS:
                getattr(self, k).copy_(st[k].to(self._dev))
            if self.norm_count is not None and "norm_count" in st:
                self.norm_count.copy_(st["norm_count"].to(self._dev))
        self._step0, self._seed, self._perm_round = int(st["step0"]), int(st["seed"]), int(st.get("perm_round", 0))


def _split(reward_net) -> Tuple[Any, Any]:
    """(output normaliser or None, the reward net under it)."""
    if isinstance(reward_net, reward_nets.NormalizedRewardNet):
        return reward_net.normalize_output_layer, reward_net.base
    return None, reward_net


def rollout_reward_mlp_ok(seq: nn.Sequential) -> Tuple[bool, str]:
    """Whether the rollout's reward pass can evaluate this ``build_mlp`` Sequential (reason when not)."""
    try:
        norm, lins, _, _ = _mlp_layers(seq)
    except ValueError as e:
        return False, str(e)
    if norm is not None and not isinstance(norm, networks.BaseNorm):
        return False, "unsupported input normaliser"
    if len(lins) > 4 or max([lins[0].in_features] + [l.out_features for l in lins]) > 64:
        return False, "reward MLP too wide / deep for the rollout kernel"
    return True, ""


class OutputNormMixin:
    """``NormalizedRewardNet.predict_processed`` (update_stats=True) replayed on device after
    the rollout kernel: the kernel stores the raw learned reward and the TimeLimit
    bootstrap; ``reward_outnorm`` normalises step by step in env order and Chan-merges each
    step's moments (all-reduced once per round under DP)."""

    def _output_norm(self):
        return _split(self._reward_net)[0]

    def _rollout_extra_bufs(self) -> Dict[str, Any]:
        out_norm = self._output_norm()
        if out_norm is None:
            return {}
        if not hasattr(self, "_rew_raw"):
            self._rew_raw = th.zeros(self.T, self.N, device=self._dev)
            self._onorm_count = th.zeros(1, device=self._dev)
        return {"rew_raw": self._rew_raw}

    @profiling.traced("rollout/reward_outnorm")
    def _post_rollout_rewards(self) -> None:
        out_norm = self._output_norm()
        if out_norm is None:
            return
        step_stats = None
        if pdist.norm_sync_active():
            raw = self._rew_raw.double()
            msg = th.stack([th.full((self.T,), float(self.N), dtype=th.float64, device=self._dev),
                            raw.sum(1), raw.square().sum(1)], 1).contiguous()
            pdist.allreduce_sum_(msg)
            cnt = msg[:, 0]
            mean = msg[:, 1] / cnt
            var = (msg[:, 2] / cnt - mean * mean).clamp_min(0.0)
            step_stats = th.stack([cnt, mean, var], 1).float().contiguous()
        # an int32 module count is read / written by the kernel itself (no copies around it)
        direct = out_norm.count.dtype == th.int32
        if not direct:
            self._onorm_count.copy_(out_norm.count.reshape(1))
        self._C.engine_reward_outnorm(dict(T=self.T, N=self.N, rew_raw=self._rew_raw, boot=self._boot,
                                           rewards=self.buf["rewards"], mean=out_norm.running_mean,
                                           var=out_norm.running_var, count=self._onorm_count,
                                           count_i=out_norm.count if direct else None,
                                           eps=float(out_norm.eps), step_stats=step_stats))
        if not direct:
            out_norm.count.copy_(self._onorm_count.to(out_norm.count.dtype).reshape(()))

