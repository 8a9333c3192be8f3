"""Device-resident AIRL -- the GAIL device engine with AIRL's reward and discriminator.

Reference: ``src/imitation/algorithms/adversarial/airl.py``. What changes
with respect to :class:`~imitation_amd.engine.gail.DeviceGAIL`:

* generator reward = ``reward_train`` = the shaped reward net itself
  (``airl.py:121-124``): the rollout kernel evaluates ``r(s, a) + gamma (1 - d) Phi(s') -
  Phi(s)`` (``reward_nets.py:701-736``, base MLP and potential MLP, both with their own
  input RunningNorm, evaluation mode) for every env step, in registers;
* ``NormalizedRewardNet`` output normalisation (``reward_nets.py:637-671``): the reference
  normalises each env step's rewards with the running statistics and then merges that
  step's batch moments -- a sequential dependency across the whole rollout. The rollout
  kernel stores the raw shaped reward and the TimeLimit bootstrap separately and one
  wave (``reward_outnorm``) replays the merge in env order: exactly the reference's
  per-step result, with the moments of each step all-reduced in ONE collective per round
  under data parallelism;
* discriminator logit ``r(s,a,s',d) - log pi(a|s)`` (``airl.py:114-119``): a fused update
  (``csrc/kernels/airl_disc.hip``, :class:`AirlDiscPlan`) -- per minibatch one gather, one
  norm launch (the policy, base and potential RunningNorm merges in the reference's order:
  potential on s' then on s) and one fwd/loss/bwd launch (policy log-prob, base reward,
  both potential passes, BCE + statistics, backward of the base and potential MLPs), then
  one fixed-order Adam launch -- instead of ~60 autograd launches. Configurations outside
  the kernel's limits keep the generic (graphed autograd) update.

PPO (MlpPolicy [64, 64], minibatch 512 in the tuned Hopper config) runs on the
cooperating-workgroup register-chained kernel.
"""

from __future__ import annotations

import os
from typing import Any, Dict, List, Optional, Tuple

import torch as th
from numpy import prod as np_prod

from imitation_amd.algorithms.adversarial.airl import AIRL
from imitation_amd.engine.adversarial import DeviceEngineMixin
from imitation_amd.engine.generator import (OutputNormMixin, _mlp_layers, _policy_nets, _split, rollout_reward_mlp_ok,
                                            supports_generator)
from imitation_amd.parallel import dist as pdist
from imitation_amd.rewards import reward_nets
from imitation_amd.util import networks
from imitation_amd.utils import profiling


def supports(venv, gen_algo, reward_net) -> Tuple[bool, str]:
    ok, why = supports_generator(venv, gen_algo)
    if not ok:
        return ok, why
    out_norm, shaped = _split(reward_net)
    if out_norm is not None and type(out_norm) is not networks.RunningNorm:
        return False, "output normaliser is not RunningNorm"
    if not isinstance(shaped, reward_nets.ShapedRewardNet):
        return False, "reward net is not a ShapedRewardNet"
    if not isinstance(shaped.base, reward_nets.BasicRewardNet):
        return False, "shaped base is not a BasicRewardNet"
    if not isinstance(shaped.potential, reward_nets.BasicPotentialMLP):
        return False, "potential is not a BasicPotentialMLP"
    D = int(np_prod(venv.observation_space.shape))
    try:
        plins = _mlp_layers(shaped.potential._potential_net)[1]
    except ValueError as e:
        return False, str(e)
    if plins[0].in_features != D or plins[-1].out_features != 1:
        return False, "potential MLP shape"
    for seq in (shaped.base.mlp, shaped.potential._potential_net):
        ok, why = rollout_reward_mlp_ok(seq)
        if not ok:
            return ok, why
    return True, ""


class DeviceAIRL(OutputNormMixin, DeviceEngineMixin, AIRL):
    """AIRL whose generator rounds run entirely on the GPU (see module docstring)."""

    _host_cls_name = "algorithms.adversarial.airl.AIRL"

    _supports = staticmethod(supports)

    def _reward_spec(self) -> Dict[str, Any]:
        _, shaped = _split(self._reward_net)
        base = shaped.base
        rnorm, rl, rh, ro = _mlp_layers(base.mlp)
        pnorm, pl, ph, po = _mlp_layers(shaped.potential._potential_net)
        return dict(rew=self._wave_mlp(rl, rh, ro, rnorm), pot=self._wave_mlp(pl, ph, po, pnorm), shaped=1,
                    shaping_gamma=float(shaped.discount_factor), rew_transform=0, use_state=int(base.use_state),
                    use_action=int(base.use_action), use_next_state=int(base.use_next_state),
                    use_done=int(base.use_done))

    # ------------------------------------------------------------------ fused discriminator (airl_disc.hip)
    #: log pi needs the post-PPO policy: the updates follow PPO on the main stream, but the round is
    #: pipelined like GAIL's (_overlapped_round: PPO stats copied async, the updates and the next
    #: rollout enqueued before the host reads anything); IMITATION_AMD_DISC_OVERLAP=0: serial
    _disc_on_main = True

    def _fused_disc_check(self) -> Tuple[bool, str]:
        if os.environ.get("IMITATION_AMD_AIRL_FUSED", "1") == "0":
            return False, "disabled (IMITATION_AMD_AIRL_FUSED=0)"
        ok, why = self._common_disc_check(AIRL)
        if not ok:
            return ok, why
        _, shaped = _split(self._reward_net)
        try:
            bnorm, blins, _, bout = _mlp_layers(shaped.base.mlp)
            pnorm, plins, _, pout = _mlp_layers(shaped.potential._potential_net)
            qnorm, qlins, _, _ = _policy_nets(self.gen_algo.policy)
        except ValueError as e:
            return False, str(e)
        for norm in (bnorm, pnorm, qnorm):
            if norm is not None and type(norm) is not networks.RunningNorm:
                return False, "a normaliser is not RunningNorm"
        if bout != 0 or pout != 0 or blins[-1].out_features != 1 or plins[-1].out_features != 1:
            return False, "reward / potential MLP shape"
        if len(blins) > 4 or len(plins) > 4 or len(qlins) > 4:
            return False, "MLP deeper than 4 layers"
        widths = [l.out_features for l in blins + plins + qlins] + [blins[0].in_features, plins[0].in_features,
                                                                    qlins[0].in_features]
        if max(widths) > 64 or self.A > 16:
            return False, "MLP wider than 64"
        if not self._reward_params_are(blins + plins):
            return False, "reward net has parameters outside its MLPs"
        base = shaped.base
        din = (base.use_state + base.use_next_state) * self.D + base.use_action * self.A + base.use_done
        if din + 2 * self.D > 128:
            return False, "too many input columns"
        # every weight and row image of the three nets is resident in LDS at once: deep or wide
        # combinations inside the limits above can still be over it
        dims = [[l.in_features for l in lins] + [lins[-1].out_features] for lins in (qlins, blins, plins)]
        if self._C.airl_plan_lds_bytes(*dims) < 0:
            return False, "MLP images over the fused kernel's LDS limit"
        return True, ""

    def _setup_disc_plan(self) -> None:
        dev = self._dev
        _, shaped = _split(self._reward_net)
        base = shaped.base
        bnorm, blins, bh, _ = _mlp_layers(base.mlp)
        pnorm, plins, ph, _ = _mlp_layers(shaped.potential._potential_net)
        qnorm, qlins, _, qh = _policy_nets(self.gen_algo.policy)
        self._bnorm, self._pnorm = bnorm, pnorm
        ed = self._setup_disc_params(blins + plins)
        n = self._rflat.n
        gd = self._gen_dev._arrays
        B, mb = self.demo_batch_size, self.demo_minibatch_size
        gblk, fblk = self._C.airl_plan_sizes(mb)
        din = blins[0].in_features
        D = self.D
        ncol = din + 2 * D
        z = lambda *sh, dt=th.float32: th.zeros(*sh, device=dev, dtype=dt)  # noqa: E731
        rows = 2 * mb
        self._disc_ws = dict(Xb=z(rows * din), S=z(rows * D), S2=z(rows * D), Act=z(rows * (1 if self.discrete else self.A)),
                             Done=z(rows), partials=z(self._C.airl_partials_floats(mb, ncol)), sums=z(2 * ncol, dt=th.float64), nrm=z(4 * 256),
                             slab=z((B // mb) * fblk * n), stats_slab=z((B // mb) * fblk * 8), grads=z(n))
        g = self._disc_opt.param_groups[0]
        pol = self.gen_algo.policy

        def net(lins, act):
            return dict(W=[l.weight for l in lins], b=[l.bias for l in lins], hidden_act=int(act))

        def norm_args(prefix, nm):
            if nm is None:
                return {f"{prefix}_mean": None, f"{prefix}_var": None, f"{prefix}_count": None, f"eps_{prefix}": 1e-5}
            return {f"{prefix}_mean": nm.running_mean, f"{prefix}_var": nm.running_var, f"{prefix}_count": nm.count,
                    f"eps_{prefix}": float(nm.eps)}

        d = dict(batch=B, minibatch=mb, obs_dim=D, act_dim=self.A, act_discrete=int(self.discrete),
                 use_state=int(base.use_state), use_action=int(base.use_action), use_next_state=int(base.use_next_state),
                 use_done=int(base.use_done), e_obs=ed["obs"], e_next_obs=ed["next_obs"], e_acts=ed["acts"],
                 e_dones=ed["dones"], g_obs=gd["obs"], g_next_obs=gd["next_obs"], g_acts=gd["acts"], g_dones=gd["dones"],
                 pol=net(qlins, qh), base=net(blins, bh), pot=net(plins, ph),
                 log_std=pol.log_std if self.has_log_std else None, gamma=float(shaped.discount_factor),
                 params=self._rflat.flat, exp_avg=self._r_m, exp_avg_sq=self._r_v, beta1=float(g["betas"][0]),
                 beta2=float(g["betas"][1]), eps=float(g["eps"]), weight_decay=float(g.get("weight_decay", 0.0)),
                 **norm_args("b", bnorm), **norm_args("p", pnorm), **norm_args("q", qnorm), **self._disc_ws)
        self._disc_plan = self._C.AirlDiscPlan(d)
        # split rounds (single rank): the updates' gathers + norm merges are staged on the main
        # stream right after PPO, then the next rollout's step chain runs concurrently with the
        # fwd/bwd + Adam applies on the side stream (see _split_round)
        # (data parallel too: the staging's normaliser all-reduces run on the main stream, the
        # applies' gradient all-reduces on the side stream, where nothing else uses the
        # communicator while they run -- the next step chain has no collectives)
        self._disc_split = (self._overlap_disc and os.environ.get("IMITATION_AMD_AIRL_SPLIT", "1") != "0")
        if self._disc_split:
            self._disc_plan.reserve(max(1, self.n_disc_updates_per_round))
        self._q_deferred, self._q_defer_rows = False, 0  # _stage_disc_updates
        self._early_staged_rounds = 0  # _split_round

    def _disc_merges(self) -> Tuple[bool, bool, bool]:
        """Which of the base, potential and policy RunningNorms merge an update's batch."""
        return (self._bnorm is not None and self._bnorm.training, self._pnorm is not None and self._pnorm.training,
                self.pol_norm is not None and self.pol_norm.training)

    @profiling.traced("disc/update")
    def _fused_disc_update(self, slot: int, defer_pol: bool = False, e_idx: Optional[th.Tensor] = None,
                           g_idx: Optional[th.Tensor] = None, apply: bool = True) -> None:
        """One discriminator optimizer step (== AdversarialTrainer.train_disc with AIRL's logits)
        on the fused kernels, with no host sync. ``e_idx`` / ``g_idx``: explicit expert / replay
        rows (tests); ``apply=False`` stops after the gradient reduction (``_disc_ws["grads"]``)."""
        self._run_disc_update(slot, self._disc_merges(), e_idx, g_idx, apply)

    @profiling.traced("disc/stage")
    def _stage_disc_updates(self, n: int, defer_q: bool = False) -> List[Tuple[float, float]]:
        """The gathers and RunningNorm merges (policy, base, potential) of the round's ``n``
        updates, in update order (``AirlDiscPlan.stage``): everything of an update that the
        norms see, none of it dependent on the discriminator weights. Returns each update's
        Adam (step_size, sqrt(1 - beta2^t)).

        ``defer_q``: leave the policy-norm merges to ``_merge_deferred_q`` (one launch after
        PPO), so the staging can run on the side stream during the PPO update (under DP its
        normaliser all-reduces then run there too); ``self._q_deferred`` says whether there is
        anything to merge."""
        # (grows only here: the previous round's applies were waited for on the host)
        self._disc_plan.reserve(max(1, n))
        self._adopt_disc_opt_state()
        merges = self._disc_merges()
        scal = []
        world = pdist.world_size()
        defer_q = defer_q and merges[2]
        self._q_deferred = defer_q
        synced = world > 1 and pdist.norm_sync_active()
        mb = self.demo_minibatch_size
        self._q_defer_rows = 2 * mb * (world if synced else 1)
        cur = th.cuda.current_stream(self._dev)
        for i in range(n):
            e_idx, g_idx = self._draw_disc_indices()
            # the epoch permutation may come from another stream's pool: keep its block alive
            # for this stream's reads
            e_idx.record_stream(cur)
            if not synced:
                self._disc_plan.stage(i, e_idx, g_idx, *merges, defer_q)
            else:  # the DP update's order: gather, moments, all-reduce, merges -- per minibatch
                for k in range(self.demo_batch_size // mb):
                    self._disc_plan.stage_part(i, k, e_idx, g_idx, 1, 0, *merges)
                    pdist.allreduce_sum_(self._disc_ws["sums"])
                    self._disc_plan.stage_part(i, k, e_idx, g_idx, 2, 2 * mb * world, *merges, defer_q)
            scal.append(self._adam_scalars(i + 1))
        return scal

    def _merge_deferred_q(self, n: int) -> None:
        """The policy-norm merges ``_stage_disc_updates(n, defer_q=True)`` left (update order)."""
        if self._q_deferred:
            self._disc_plan.q_merge(n, self._q_defer_rows)
            self._q_deferred = False

    @profiling.traced("disc/apply")
    def _apply_disc_updates(self, scal: List[Tuple[float, float]], steps: List[int]) -> None:
        """The fwd/bwd passes and Adam steps of the staged updates (``AirlDiscPlan.apply``)."""
        world = pdist.world_size()
        for i, (step_size, bc2_sqrt) in enumerate(scal):
            if world == 1:
                self._disc_plan.apply(i, step_size, bc2_sqrt, self._disc_stats[i])
            else:  # mean gradient over ranks between the reduction and Adam (one-shot, in stream order)
                self._disc_plan.apply_grads(i, self._disc_stats[i])
                pdist.allreduce_grads_flat(self._disc_ws["grads"])
                self._disc_plan.adam(0, 1, step_size, bc2_sqrt, None)
            self._bump_disc_step()
            steps.append(self._disc_step)

    # ------------------------------------------------------------------ split rounds
    def _after_ppo(self, n: int, ready: th.cuda.Event, launch_next: bool, defer_pol: bool):
        if self._disc_split and n > 0:
            return self._split_round(n, launch_next)
        return super()._after_ppo(n, ready, launch_next, defer_pol)

    def _stage_during_ppo(self) -> bool:
        """Split-round staging on the side stream, concurrent with PPO. Under data parallelism
        only with the replicated PPO update, which issues no collective: the staging's normaliser
        all-reduces are then the only users of the communicator while they run.
        IMITATION_AMD_AIRL_EARLY_STAGE=0: stage behind PPO on the main stream."""
        return ((pdist.world_size() == 1 or self._dp_replicated) and self._host_staged
                and os.environ.get("IMITATION_AMD_AIRL_EARLY_STAGE", "1") != "0")

    def _split_round(self, n: int, launch_next: bool) -> Tuple[List[int], Optional[th.cuda.Event]]:
        """Rest of a split round after PPO (instead of the mixin's ``_after_ppo``). The updates'
        gathers + norm merges are the only part of them that the next rollout's step chain depends
        on (through the policy RunningNorm): stage them on the main stream, apply the updates
        (fwd/bwd + Adam) on the side stream while that step chain runs, then the rollout's reward
        pass behind the applies."""
        main = th.cuda.current_stream(self._dev)
        side = self._side_stream
        ppo_done = self._ppo_done
        steps: List[int] = []
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
            self._early_staged_rounds += 1
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
        self._wait_ev(main, disc_dev)
        if launch_next:
            reward = not self.debug_use_ground_truth
            self._launch_post(reward)
            if reward:
                self._post_rollout_rewards()
            nxt = self._stage_rollout_to_host()
        ppo_done.synchronize()
        self._log_gen()
        disc_done.synchronize()
        return steps, nxt
