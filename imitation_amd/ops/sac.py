"""Fused SAC update: every gradient step of one ``SAC.train`` call in ONE launch.

``sac_update_step`` runs ``G`` gradient steps of Soft Actor-Critic on flat buckets: the actor
(two-hidden-layer ReLU trunk, ``mu`` / ``log_std`` heads), the twin critics and, when it is
learned, ``log_ent_coef`` each in a :class:`~imitation_amd.ops.optim.FusedAdam` bucket, and the
target critics in one flat buffer. A step gathers its batch rows by flat row id from one or two
replay rings (the agent ring and SQIL's expert ring), samples the actor on ``next_obs`` and
``obs`` with the given noise, forms the soft target, updates the critics, updates the actor
through the updated critics, updates the entropy coefficient and Polyak-averages the target --
``csrc/kernels/sac_update.hip``, one workgroup, all fp32.

``sac_update_reference`` is the same ``G`` steps hand-written in torch ops on the same buckets,
row ids and noise (any float dtype, CPU or GPU): the numerics oracle of the kernel tests and what
``sac_update_step`` runs for CPU tensors.
"""

from __future__ import annotations

import dataclasses
import math
from typing import Any, Dict, List, Mapping, Optional, Sequence, Tuple

import torch as th

from imitation_amd import ops
from imitation_amd.ops.optim import FusedAdam

MAX_DIM = 64  # obs dim, hidden widths, obs dim + action dim
MAX_BATCH = 256  # rows per gradient step
LOG_STD_MIN, LOG_STD_MAX = -20.0, 2.0
_HALF_LOG_2PI = 0.5 * math.log(2.0 * math.pi)
_SQUASH_EPS = 1e-6

# a replay ring as flat rows: (obs [SN, D], next_obs [SN, D], actions [SN, A] float, rewards [SN],
# dones [SN], timeouts [SN]); the effective done of a row is ``done * (1 - timeout)``
Source = Sequence[th.Tensor]
# a FusedAdam group's flat state: {"flat", "grad", "m", "v", "step"}
Bucket = Mapping[str, th.Tensor]
# (lr, beta1, beta2, eps) of a bucket's Adam
AdamHP = Tuple[float, float, float, float]
DEFAULT_HP: AdamHP = (3e-4, 0.9, 0.999, 1e-8)
OUTPUTS = ("critic_loss", "actor_loss", "ent_coef", "ent_coef_loss")


def _offsets(sizes: Sequence[int]) -> Tuple[int, ...]:
    offs, off = [], 0
    for s in sizes:
        offs.append(off)
        off += s
    return tuple(offs)


@dataclasses.dataclass(frozen=True)
class SACLayout:
    """Shapes of the actor ``D -> aH1 -> aH2 -> (mu, log_std) [A]`` and of each critic
    ``D + A -> cH1 -> cH2 -> 1``, and the offsets of their tensors in the flat buckets, in
    ``parameters()`` order: the actor's ``W1, b1, W2, b2, Wmu, bmu, Wls, bls``; the critics'
    ``W1, b1, W2, b2, W3, b3`` of ``qf0``, then of ``qf1``."""

    D: int
    A: int
    actor_arch: Tuple[int, int]
    critic_arch: Tuple[int, int]
    actor_offsets: Tuple[int, ...]
    critic_offsets: Tuple[int, ...]

    @staticmethod
    def _actor_shapes(D, A, arch):
        H1, H2 = arch
        return [(H1, D), (H1,), (H2, H1), (H2,), (A, H2), (A,), (A, H2), (A,)]

    @staticmethod
    def _critic_shapes(D, A, arch):
        H1, H2 = arch
        return [(H1, D + A), (H1,), (H2, H1), (H2,), (1, H2), (1,)] * 2

    @classmethod
    def from_dims(cls, D: int, A: int, actor_arch: Sequence[int], critic_arch: Optional[Sequence[int]] = None) -> "SACLayout":
        actor_arch = tuple(int(w) for w in actor_arch)
        critic_arch = actor_arch if critic_arch is None else tuple(int(w) for w in critic_arch)
        if len(actor_arch) != 2 or len(critic_arch) != 2:
            raise ValueError("SACLayout needs two hidden layers in the actor and in the critics")
        a_sizes = [math.prod(s) for s in cls._actor_shapes(D, A, actor_arch)]
        c_sizes = [math.prod(s) for s in cls._critic_shapes(D, A, critic_arch)]
        return cls(int(D), int(A), actor_arch, critic_arch, _offsets(a_sizes), _offsets(c_sizes))

    @classmethod
    def from_params(cls, actor_params: Sequence[th.Tensor], critic_params: Sequence[th.Tensor]) -> "SACLayout":
        ap, cp = list(actor_params), list(critic_params)
        if len(ap) != 8 or [p.dim() for p in ap] != [2, 1] * 4:
            raise ValueError("SACLayout needs the eight actor parameters W1, b1, W2, b2, Wmu, bmu, Wls, bls")
        if len(cp) != 12 or [p.dim() for p in cp] != [2, 1] * 6:
            raise ValueError("SACLayout needs the 2 x 6 critic parameters W1, b1, W2, b2, W3, b3")
        (H1, D), (H2, K2), (A, K3) = ap[0].shape, ap[2].shape, ap[4].shape
        (C1, DA), (C2, _), _ = cp[0].shape, cp[2].shape, cp[4].shape
        L = cls.from_dims(int(D), int(A), (int(H1), int(H2)), (int(C1), int(C2)))
        if K2 != H1 or K3 != H2 or DA != D + A:
            raise ValueError("SACLayout: layer shapes do not chain")
        if [tuple(p.shape) for p in ap] != L._actor_shapes(L.D, L.A, L.actor_arch):
            raise ValueError("SACLayout: unexpected actor parameter shapes")
        if [tuple(p.shape) for p in cp] != L._critic_shapes(L.D, L.A, L.critic_arch):
            raise ValueError("SACLayout: unexpected critic parameter shapes")
        return L

    @property
    def n_actor(self) -> int:
        return self.actor_offsets[7] + self.A

    @property
    def n_critic(self) -> int:
        return self.critic_offsets[11] + 1

    @property
    def dims(self) -> List[int]:
        return [self.D, self.A, *self.actor_arch, *self.critic_arch]

    @staticmethod
    def _views(flat, offsets, shapes):
        return [flat[o : o + math.prod(s)].view(s) for o, s in zip(offsets, shapes)]

    def actor_views(self, flat: th.Tensor) -> List[th.Tensor]:
        """``(W1, b1, W2, b2, Wmu, bmu, Wls, bls)`` as views of ``flat``."""
        return self._views(flat, self.actor_offsets, self._actor_shapes(self.D, self.A, self.actor_arch))

    def critic_views(self, flat: th.Tensor) -> List[List[th.Tensor]]:
        """``[(W1, b1, W2, b2, W3, b3) of qf0, ... of qf1]`` as views of ``flat``."""
        v = self._views(flat, self.critic_offsets, self._critic_shapes(self.D, self.A, self.critic_arch))
        return [v[:6], v[6:]]


def _outputs(G: int, like: th.Tensor, outs) -> Dict[str, th.Tensor]:
    if outs is None:
        outs = {}
    # (every step writes all four: no fill needed)
    return {k: outs[k] if outs.get(k) is not None else th.empty(G, dtype=like.dtype, device=like.device) for k in OUTPUTS}


def _group(hp: AdamHP) -> Dict[str, Any]:
    return {"lr": hp[0], "betas": (hp[1], hp[2]), "eps": hp[3], "weight_decay": 0.0, "maximize": False,
            "decoupled_weight_decay": False}


def _adam(hp: AdamHP, f: Bucket) -> None:
    """One Adam step of the bucket from its gradient, which stays in the bucket."""
    kept = f["grad"].clone()
    f["step"].add_(1.0)
    FusedAdam._step_reference(_group(hp), f)  # (clears the gradient it consumed)
    f["grad"].copy_(kept)


def actor_sample(av: Sequence[th.Tensor], x: th.Tensor, eps: th.Tensor):
    """The actor on ``x`` with noise ``eps``: ``(action, logp, (h1, h2, raw log_std, std))``."""
    W1, b1, W2, b2, Wm, bm, Wl, bl = av
    h1 = th.relu(x @ W1.T + b1)
    h2 = th.relu(h1 @ W2.T + b2)
    mu, raw = h2 @ Wm.T + bm, h2 @ Wl.T + bl
    ls = raw.clamp(LOG_STD_MIN, LOG_STD_MAX)
    std = ls.exp()
    act = th.tanh(mu + std * eps)
    logp = (-0.5 * eps * eps - ls - _HALF_LOG_2PI).sum(1) - th.log(1 - act * act + _SQUASH_EPS).sum(1)
    return act, logp, (h1, h2, raw, std)


def critic_q(cv: Sequence[th.Tensor], x: th.Tensor):
    """One critic on ``x = [obs | action]``: ``(q [B, 1], h1, h2)``."""
    W1, b1, W2, b2, W3, b3 = cv
    h1 = th.relu(x @ W1.T + b1)
    h2 = th.relu(h1 @ W2.T + b2)
    return h2 @ W3.T + b3, h1, h2


def sac_update_reference(src_a: Source, src_b: Optional[Source], ids_a: th.Tensor, ids_b: Optional[th.Tensor],
                         eps_pi: th.Tensor, eps_next: th.Tensor, actor: Bucket, critic: Bucket, ent: Optional[Bucket],
                         target: th.Tensor, layout: SACLayout, actor_hp: AdamHP = DEFAULT_HP, critic_hp: AdamHP = DEFAULT_HP,
                         ent_hp: AdamHP = DEFAULT_HP, ent_coef: float = 1.0, target_entropy: float = -1.0,
                         gamma: float = 0.99, tau: float = 0.005, target_update_interval: int = 1,
                         outs: Optional[Dict[str, th.Tensor]] = None,
                         info: Optional[List[Dict[str, th.Tensor]]] = None) -> Dict[str, th.Tensor]:
    """The ``G = ids_a.shape[0]`` gradient steps in torch ops, in the dtype of ``actor["flat"]``.
    Updates the buckets (``ent``: the ``log_ent_coef`` bucket, or None for the fixed ``ent_coef``)
    and ``target`` in place, leaves the last step's gradients in the ``grad`` buffers and returns
    ``{critic_loss, actor_loss, ent_coef, ent_coef_loss}``, each ``[G]``. ``info``: a list that
    receives per step the branch-point values (``q_next``, ``q_pi`` ``[B, 2]`` and the raw
    ``log_std`` of both actor forwards)."""
    G = int(ids_a.shape[0])
    flat = actor["flat"]
    outs = _outputs(G, flat, outs)
    n_e = 0 if ids_b is None else int(ids_b.shape[1])
    L = layout
    av, ag = L.actor_views(actor["flat"]), L.actor_views(actor["grad"])
    cv, cg = L.critic_views(critic["flat"]), L.critic_views(critic["grad"])
    tv = L.critic_views(target)
    with th.no_grad():
        for g in range(G):
            parts = [[t[ids_a[g]] for t in src_a]]
            if n_e:
                parts.append([t[ids_b[g]] for t in src_b])
            obs, next_obs, act, rew, done, tmo = (th.cat([p[i] for p in parts]) for i in range(6))
            B = obs.shape[0]
            obs, next_obs, act = obs.reshape(B, -1), next_obs.reshape(B, -1), act.reshape(B, -1)
            d = (done * (1 - tmo)).reshape(B, 1)
            if ent is not None:
                log_ent = ent["flat"][0].clone()
                coef = log_ent.exp()
            else:
                coef = th.as_tensor(ent_coef, dtype=flat.dtype, device=flat.device)
            outs["ent_coef"][g] = coef
            # ---- actor on obs, the entropy coefficient's loss and step
            a_pi, logp, (h1, h2, raw, std) = actor_sample(av, obs, eps_pi[g])
            if ent is not None:
                mean = (logp + target_entropy).mean()
                outs["ent_coef_loss"][g] = -(log_ent * mean)
                ent["grad"].zero_()
                ent["grad"][0] = -mean
                _adam(ent_hp, ent)
            else:
                outs["ent_coef_loss"][g] = 0.0
            # ---- target
            a_next, logp_next, (_, _, raw_next, _) = actor_sample(av, next_obs, eps_next[g])
            xn = th.cat([next_obs, a_next], dim=1)
            q_next = th.cat([critic_q(tv[k], xn)[0] for k in range(2)], dim=1)
            y = rew.reshape(B, 1) + (1 - d) * gamma * (q_next.min(dim=1, keepdim=True).values - coef * logp_next.reshape(B, 1))
            # ---- critic update
            x = th.cat([obs, act], dim=1)
            loss = 0.0
            for k in range(2):
                W1, b1, W2, b2, W3, b3 = cv[k]
                q, c1, c2 = critic_q(cv[k], x)
                delta = q - y
                loss = loss + (delta * delta).mean()
                dq = delta / B
                dz2 = (dq @ W3) * (c2 > 0)
                dz1 = (dz2 @ W2) * (c1 > 0)
                for dst, val in zip(cg[k], (dz1.T @ x, dz1.sum(0), dz2.T @ c1, dz2.sum(0), dq.T @ c2, dq.sum(0))):
                    dst.copy_(val)
            outs["critic_loss"][g] = 0.5 * loss
            _adam(critic_hp, critic)
            # ---- actor update through the updated critics: dq / da of the smaller one per row
            xp = th.cat([obs, a_pi], dim=1)
            qs, dqda = [], []
            for k in range(2):
                W1, b1, W2, b2, W3, b3 = cv[k]
                q, c1, c2 = critic_q(cv[k], xp)
                qs.append(q)
                dqda.append((((W3 * (c2 > 0)) @ W2) * (c1 > 0)) @ W1[:, L.D :])
            q_pi = th.cat(qs, dim=1)
            first = q_pi[:, :1] <= q_pi[:, 1:]
            outs["actor_loss"][g] = (coef * logp.reshape(B, 1) - q_pi.min(dim=1, keepdim=True).values).mean()
            om = 1 - a_pi * a_pi
            dLda = (coef * (2 * a_pi / (om + _SQUASH_EPS)) - th.where(first, dqda[0], dqda[1])) / B
            dmu = dLda * om
            dls = (dmu * (std * eps_pi[g]) - coef / B) * ((raw >= LOG_STD_MIN) & (raw <= LOG_STD_MAX))
            W1, b1, W2, b2, Wm, bm, Wl, bl = av
            dz2 = (dmu @ Wm + dls @ Wl) * (h2 > 0)
            dz1 = (dz2 @ W2) * (h1 > 0)
            for dst, val in zip(ag, (dz1.T @ obs, dz1.sum(0), dz2.T @ h1, dz2.sum(0), dmu.T @ h2, dmu.sum(0), dls.T @ h2,
                                     dls.sum(0))):
                dst.copy_(val)
            _adam(actor_hp, actor)
            # ---- Polyak
            if g % target_update_interval == 0:
                target.mul_(1 - tau).add_(critic["flat"], alpha=tau)
            if info is not None:
                info.append(dict(q_next=q_next.clone(), q_pi=q_pi.clone(), raw=raw.clone(), raw_next=raw_next.clone()))
    return outs


def _bucket_list(f: Bucket) -> List[th.Tensor]:
    return [f["flat"], f["grad"], f["m"], f["v"], f["step"]]


def sac_update_step(src_a: Source, src_b: Optional[Source], ids_a: th.Tensor, ids_b: Optional[th.Tensor],
                    eps_pi: th.Tensor, eps_next: th.Tensor, actor: Bucket, critic: Bucket, ent: Optional[Bucket],
                    target: th.Tensor, layout: SACLayout, actor_hp: AdamHP = DEFAULT_HP, critic_hp: AdamHP = DEFAULT_HP,
                    ent_hp: AdamHP = DEFAULT_HP, ent_coef: float = 1.0, target_entropy: float = -1.0, gamma: float = 0.99,
                    tau: float = 0.005, target_update_interval: int = 1,
                    outs: Optional[Dict[str, th.Tensor]] = None) -> Dict[str, th.Tensor]:
    """``G = ids_a.shape[0]`` SAC gradient steps on the flat buckets: ONE kernel launch for GPU
    tensors, :func:`sac_update_reference` for CPU tensors. ``ids_a [G, n_a]`` / ``ids_b [G, n_e]``
    are flat row ids into ``src_a`` / ``src_b`` (``src_b`` / ``ids_b`` None: one source);
    ``eps_pi`` / ``eps_next`` ``[G, n_a + n_e, A]`` the actor's noise on ``obs`` / ``next_obs``.
    Returns ``{critic_loss, actor_loss, ent_coef, ent_coef_loss}``, each ``[G]``."""
    if not ops.use_kernel(actor["flat"]):
        return sac_update_reference(src_a, src_b, ids_a, ids_b, eps_pi, eps_next, actor, critic, ent, target, layout,
                                    actor_hp, critic_hp, ent_hp, ent_coef, target_entropy, gamma, tau,
                                    target_update_interval, outs)
    outs = _outputs(int(ids_a.shape[0]), actor["flat"], outs)
    ops.native().sac_update_step(list(src_a), None if src_b is None else list(src_b), ids_a, ids_b, eps_pi, eps_next,
                                 _bucket_list(actor), [float(h) for h in actor_hp], _bucket_list(critic),
                                 [float(h) for h in critic_hp], None if ent is None else _bucket_list(ent),
                                 [float(h) for h in ent_hp], float(ent_coef), float(target_entropy), target,
                                 layout.dims, list(layout.actor_offsets), list(layout.critic_offsets), float(gamma),
                                 float(tau), int(target_update_interval), [outs[k] for k in OUTPUTS])
    return outs
