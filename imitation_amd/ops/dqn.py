"""Fused DQN TD update: every gradient step of one ``DQN.train`` call in ONE launch.

``dqn_td_step`` runs ``G`` gradient steps of a two-hidden-layer ReLU Q-network on the flat
buckets of a :class:`~imitation_amd.ops.optim.FusedAdam` (online network) and of the target
network: gather the batch rows by flat row id from one or two replay rings (the agent ring
and SQIL's expert ring), TD target, online forward, Huber loss, backward, global-norm clip
and Adam -- ``csrc/kernels/dqn_td.hip``, one workgroup, all fp32.

``dqn_td_reference`` is the same ``G`` steps in plain torch ops on the same buckets and row
ids (any float dtype, CPU or GPU): the numerics oracle of the kernel tests and what
``dqn_td_step`` runs for CPU tensors.
"""

from __future__ import annotations

import dataclasses
from typing import Optional, Sequence, Tuple

import torch as th

from imitation_amd import ops
from imitation_amd.ops.optim import FusedAdam

MAX_DIM = 64  # obs dim, hidden widths, actions
MAX_BATCH = 256  # rows per gradient step

# a replay ring as flat rows: (obs [SN, D], next_obs [SN, D], actions [SN, 1] int64, rewards [SN],
# dones [SN], timeouts [SN]); the effective done of a row is ``done * (1 - timeout)``
Source = Sequence[th.Tensor]


@dataclasses.dataclass(frozen=True)
class TDLayout:
    """Shape of the Q-network ``D -> H1 -> H2 -> A`` and the offsets of ``W1, b1, W2, b2, W3, b3``
    in a flat bucket (``q_net.parameters()`` order)."""

    D: int
    H1: int
    H2: int
    A: int
    offsets: Tuple[int, int, int, int, int, int]

    @classmethod
    def from_dims(cls, D: int, H1: int, H2: int, A: int) -> "TDLayout":
        sizes = [H1 * D, H1, H2 * H1, H2, A * H2, A]
        offs, off = [], 0
        for s in sizes:
            offs.append(off)
            off += s
        return cls(D, H1, H2, A, tuple(offs))

    @classmethod
    def from_params(cls, params: Sequence[th.Tensor]) -> "TDLayout":
        ps = list(params)
        if len(ps) != 6 or [p.dim() for p in ps] != [2, 1, 2, 1, 2, 1]:
            raise ValueError("TDLayout needs the six parameters W1, b1, W2, b2, W3, b3 of a two-hidden-layer MLP")
        (H1, D), (H2, K2), (A, K3) = ps[0].shape, ps[2].shape, ps[4].shape
        if K2 != H1 or K3 != H2 or [p.numel() for p in ps[1::2]] != [H1, H2, A]:
            raise ValueError("TDLayout: layer shapes do not chain")
        return cls.from_dims(int(D), int(H1), int(H2), int(A))

    @property
    def n(self) -> int:
        return self.offsets[5] + self.A

    def views(self, flat: th.Tensor):
        """``(W1, b1, W2, b2, W3, b3)`` as views of ``flat``."""
        o = self.offsets
        shapes = [(self.H1, self.D), (self.H1,), (self.H2, self.H1), (self.H2,), (self.A, self.H2), (self.A,)]
        out = []
        for off, shp in zip(o, shapes):
            k = 1
            for s in shp:
                k *= s
            out.append(flat[off : off + k].view(shp))
        return out


def _outputs(G: int, like: th.Tensor, losses, gnorm):
    if losses is None:
        losses = th.empty(G, dtype=like.dtype, device=like.device)
    if gnorm is None:
        gnorm = th.empty(G, dtype=like.dtype, device=like.device)
    return losses, gnorm


def dqn_td_reference(src_a: Source, src_b: Optional[Source], ids_a: th.Tensor, ids_b: Optional[th.Tensor], flat: th.Tensor,
                     grad: th.Tensor, exp_avg: th.Tensor, exp_avg_sq: th.Tensor, step: th.Tensor, target: th.Tensor,
                     layout: TDLayout, lr: float, betas=(0.9, 0.999), eps: float = 1e-8, gamma: float = 0.99,
                     max_norm: float = 10.0, losses: Optional[th.Tensor] = None, gnorm: Optional[th.Tensor] = None):
    """The ``G = ids_a.shape[0]`` gradient steps in torch ops, in the dtype of ``flat``. Updates
    ``flat``, the moments and ``step`` in place, leaves the last step's clipped gradient in ``grad``
    and returns ``(losses [G], gnorm [G])`` (pre-clip norms)."""
    G = int(ids_a.shape[0])
    losses, gnorm = _outputs(G, flat, losses, gnorm)
    n_e = 0 if ids_b is None else int(ids_b.shape[1])
    group = {"betas": tuple(betas), "lr": lr, "eps": eps, "weight_decay": 0.0, "maximize": False,
             "decoupled_weight_decay": False}
    f = {"flat": flat, "grad": grad, "m": exp_avg, "v": exp_avg_sq, "step": step}
    W1, b1, W2, b2, W3, b3 = layout.views(flat)
    T1, c1, T2, c2, T3, c3 = layout.views(target)
    gW1, gb1, gW2, gb2, gW3, gb3 = layout.views(grad)
    with th.no_grad():
        for g in range(G):
            parts = [[t[ids_a[g]] for t in src_a]]
            if n_e:
                parts.append([t[ids_b[g]] for t in src_b])
            obs, next_obs, act, rew, done, tmo = (th.cat([p[i] for p in parts]) for i in range(6))
            B = obs.shape[0]
            obs, next_obs = obs.reshape(B, -1), next_obs.reshape(B, -1)
            act = act.reshape(B, 1).long()
            d = (done * (1 - tmo)).reshape(B, 1)
            next_q = th.relu(th.relu(next_obs @ T1.T + c1) @ T2.T + c2) @ T3.T + c3
            y = rew.reshape(B, 1) + (1 - d) * gamma * next_q.max(dim=1).values.reshape(B, 1)
            h1 = th.relu(obs @ W1.T + b1)
            h2 = th.relu(h1 @ W2.T + b2)
            q = h2 @ W3.T + b3
            delta = q.gather(1, act) - y
            ad = delta.abs()
            losses[g] = th.where(ad < 1, 0.5 * delta * delta, ad - 0.5).mean()  # smooth_l1_loss, beta = 1
            dq = th.zeros_like(q).scatter_(1, act, delta.clamp(-1, 1) / B)
            dz2 = (dq @ W3) * (h2 > 0)
            dz1 = (dz2 @ W2) * (h1 > 0)
            gW3.copy_(dq.T @ h2)
            gb3.copy_(dq.sum(0))
            gW2.copy_(dz2.T @ h1)
            gb2.copy_(dz2.sum(0))
            gW1.copy_(dz1.T @ obs)
            gb1.copy_(dz1.sum(0))
            norm = grad[: layout.n].norm()
            gnorm[g] = norm
            grad.mul_((max_norm / (norm + 1e-6)).clamp(max=1.0))  # clip_grad_norm_
            clipped = grad.clone()
            step.add_(1.0)
            FusedAdam._step_reference(group, f)  # (clears the gradient it consumed)
            grad.copy_(clipped)
    return losses, gnorm


def dqn_td_step(src_a: Source, src_b: Optional[Source], ids_a: th.Tensor, ids_b: Optional[th.Tensor], flat: th.Tensor,
                grad: th.Tensor, exp_avg: th.Tensor, exp_avg_sq: th.Tensor, step: th.Tensor, target: th.Tensor,
                layout: TDLayout, lr: float, betas=(0.9, 0.999), eps: float = 1e-8, gamma: float = 0.99,
                max_norm: float = 10.0, losses: Optional[th.Tensor] = None, gnorm: Optional[th.Tensor] = None):
    """``G = ids_a.shape[0]`` TD gradient steps on the flat buckets: ONE kernel launch for GPU
    tensors, :func:`dqn_td_reference` for CPU tensors. ``ids_a [G, n_a]`` / ``ids_b [G, n_e]`` are
    flat row ids into ``src_a`` / ``src_b`` (``src_b`` / ``ids_b`` None: one source). Returns
    ``(losses [G], gnorm [G])``."""
    if not ops.use_kernel(flat):
        return dqn_td_reference(src_a, src_b, ids_a, ids_b, flat, grad, exp_avg, exp_avg_sq, step, target, layout, lr,
                                betas, eps, gamma, max_norm, losses, gnorm)
    losses, gnorm = _outputs(int(ids_a.shape[0]), flat, losses, gnorm)
    ops.native().dqn_td_step(list(src_a), None if src_b is None else list(src_b), ids_a, ids_b, flat, grad, exp_avg,
                             exp_avg_sq, step, target, list(layout.offsets), layout.D, layout.H1, layout.H2, layout.A,
                             float(lr), float(betas[0]), float(betas[1]), float(eps), float(gamma), float(max_norm),
                             losses, gnorm)
    return losses, gnorm
