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
and ``train_rl`` engines. The replay store, the round scheduler and the driver of the fused
discriminator update are :class:`imitation_amd.engine.adversarial.DeviceEngineMixin`, shared with
:class:`imitation_amd.engine.airl.DeviceAIRL`; this module adds GAIL's side of that update.
"""

from __future__ import annotations

from typing import Tuple

import numpy as np
import torch as th

from imitation_amd.algorithms.adversarial.gail import GAIL
from imitation_amd.engine.adversarial import DeviceEngineMixin, flatten_order  # noqa: F401 (imported from here too)
from imitation_amd.engine.generator import _mlp_layers, _split, supports_generator
from imitation_amd.rewards import reward_nets
from imitation_amd.rl.ppo import PPO
from imitation_amd.util import networks
from imitation_amd.utils import profiling


def supports(venv, gen_algo, reward_net) -> Tuple[bool, str]:
    """Whether :class:`DeviceGAIL` can run this configuration (reason when not)."""
    ok, why = supports_generator(venv, gen_algo)
    if not ok:
        return ok, why
    if not isinstance(_split(reward_net)[1], reward_nets.BasicRewardNet):
        return False, "reward net is not a BasicRewardNet"
    return True, ""


class DeviceGAIL(DeviceEngineMixin, GAIL):
    """GAIL whose generator rounds run entirely on the GPU (see module docstring)."""

    _host_cls_name = "algorithms.adversarial.gail.GAIL"

    _supports = staticmethod(supports)

    # ------------------------------------------------------------------ fused discriminator (disc.hip)
    def _fused_disc_check(self) -> Tuple[bool, str]:
        ok, why = self._common_disc_check(GAIL)
        if not ok:
            return ok, why
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
        if not self._reward_params_are(lins):
            return False, "reward net has parameters outside its MLP"
        if self.pol_norm is not None and (type(self.pol_norm) is not networks.RunningNorm or not base.use_state):
            return False, "policy normaliser"
        return True, ""

    def _setup_disc_plan(self) -> None:
        dev = self._dev
        _, base = _split(self._reward_net)
        norm, lins, hid, _ = _mlp_layers(base.mlp)
        self._rnorm = norm
        ed = self._setup_disc_params(lins)
        n = self._rflat.n
        gd = self._gen_dev._arrays
        B, mb = self.demo_batch_size, self.demo_minibatch_size
        dims = [lins[0].in_features] + [l.out_features for l in lins]
        gblk, fblk, n_params = self._C.disc_plan_sizes(dims, mb)
        assert n_params == n, (n_params, n)
        n_mb = B // mb
        z = lambda *sh, dt=th.float32: th.zeros(*sh, device=dev, dtype=dt)  # noqa: E731
        self._disc_ws = dict(X=z(2 * mb, dims[0]), partials=z(self._C.disc_partials_floats(mb, dims[0])), slab=z(n_mb * fblk * n),
                             stats_slab=z(n_mb * fblk * 8), grads=z(n), sums=z(2 * dims[0], dt=th.float64))
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
        # the one write of an update that the concurrent PPO kernel also makes -- the policy
        # RunningNorm merge of the disc batch -- goes to this buffer (_after_ppo)
        if self._overlap_disc and self.pol_norm is not None and self._disc_plan.pol_cols > 0:
            self._ensure_pol_defer(max(1, self.n_disc_updates_per_round))

    @profiling.traced("disc/update")
    def _fused_disc_update(self, slot: int, defer_pol: bool = False) -> None:
        """One discriminator optimizer step (== AdversarialTrainer.train_disc) with no host sync.
        ``defer_pol``: record the policy-norm merges in slots ``slot * n_minibatches + k`` of
        the deferred-merge buffer instead of applying them (see :meth:`_after_ppo`)."""
        merge_rew = self._rnorm is not None and self._rnorm.training
        merge_pol = self.pol_norm is not None and self.pol_norm.training
        base = slot * self._disc_plan.n_minibatches if (defer_pol and merge_pol) else -1
        self._run_disc_update(slot, (merge_rew, merge_pol), pol_slot=base)


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
