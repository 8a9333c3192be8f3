"""Fused BC minibatch steps of a small MLP policy: ``G`` steps in ONE launch.

``bc_mlp_steps`` runs ``G`` behavioural-cloning minibatch steps of an ``ActorCriticPolicy`` whose
parameters all live in one :class:`~imitation_amd.ops.optim.FusedAdam` flat bucket: gather the
batch rows by flat row id from device-resident demonstrations, the policy trunk (two hidden
layers, Tanh or ReLU) and ``action_net``, the categorical or diagonal-Gaussian loss of
``BehaviorCloningLossCalculator`` with its seven metrics, the backward (``log_std`` included),
``l2_weight * w`` on every bucket element and Adam over the whole bucket --
``csrc/kernels/bc_mlp.hip``, one workgroup, all fp32. The value net is not evaluated (BC never
uses it); its elements get the pure L2 gradient, as they do under autograd.

``bc_mlp_reference`` is the same ``G`` steps in plain torch ops on the same buckets and row ids
(any float dtype, CPU or GPU): the numerics oracle of the kernel tests and what ``bc_mlp_steps``
runs for CPU tensors.
"""

from __future__ import annotations

import dataclasses
import math
from typing import Optional, Tuple

import torch as th
from torch import nn

from imitation_amd import ops
from imitation_amd.ops.optim import FusedAdam
from imitation_amd.ops.rl import BC_METRICS

MAX_DIM = 64  # obs dim, hidden widths, actions
MAX_BATCH = 256  # rows per minibatch
MAX_BUCKET = 64 * 1024  # elements of the flat bucket (FusedAdam's "small bucket" bound)
_HALF_LOG_2PI = 0.5 * math.log(2.0 * math.pi)


@dataclasses.dataclass(frozen=True)
class BCMlpLayout:
    """Shape of the policy path ``D -> H1 -> H2 -> A``, its head kind and trunk activation, and
    the offsets of ``W1, b1, W2, b2`` (trunk), ``W3, b3`` (``action_net``) and ``log_std`` in
    the flat bucket of ``n`` elements (padding included)."""

    D: int
    H1: int
    H2: int
    A: int
    gaussian: bool
    tanh: bool
    offsets: Tuple[int, int, int, int, int, int]
    log_std_offset: int  # -1: categorical head
    n: int

    def check(self) -> None:
        """ValueError when a size is outside the kernel's limits or a segment outside the bucket."""
        for name in ("D", "H1", "H2", "A"):
            v = getattr(self, name)
            if not 1 <= v <= MAX_DIM:
                raise ValueError(f"BCMlpLayout: {name}={v} is outside 1..{MAX_DIM}")
        if not 1 <= self.n <= MAX_BUCKET:
            raise ValueError(f"BCMlpLayout: a bucket of {self.n} elements is outside 1..{MAX_BUCKET}")
        segs = list(zip(self.offsets, self.sizes))
        if self.gaussian:
            segs.append((self.log_std_offset, self.A))
        for off, k in segs:
            if off < 0 or off + k > self.n:
                raise ValueError(f"BCMlpLayout: segment [{off}, {off + k}) is outside the bucket of {self.n} elements")

    @property
    def sizes(self) -> Tuple[int, ...]:
        return (self.H1 * self.D, self.H1, self.H2 * self.H1, self.H2, self.A * self.H2, self.A)

    @classmethod
    def from_policy(cls, policy, optimizer: FusedAdam) -> "BCMlpLayout":
        """The layout of ``policy`` in ``optimizer``'s single flat bucket. Offsets are found by
        parameter identity in ``optimizer._flat[0]``, not by an assumed order. ValueError when the
        policy path is not two Linear + Tanh/ReLU layers and a Linear head, the head is neither
        categorical nor diagonal Gaussian, or a size is outside the kernel's limits."""
        from imitation_amd.rl.distributions import CategoricalDistribution, DiagGaussianDistribution

        mods = list(policy.mlp_extractor.policy_net)
        if len(mods) != 4 or not all(isinstance(m, nn.Linear) and m.bias is not None for m in mods[0::2]):
            raise ValueError("the policy trunk is not exactly two Linear layers with an activation each")
        if type(mods[1]) is not type(mods[3]) or type(mods[1]) not in (nn.Tanh, nn.ReLU):
            raise ValueError("the policy trunk's activation is neither Tanh nor ReLU")
        head = policy.action_net
        if not isinstance(head, nn.Linear) or head.bias is None:
            raise ValueError("action_net must be a Linear layer with a bias")
        dist = policy.action_dist
        if type(dist) is DiagGaussianDistribution:
            gaussian = True
        elif type(dist) is CategoricalDistribution:
            gaussian = False
        else:
            raise ValueError(f"unsupported action distribution {type(dist).__name__}")
        l1, l2 = mods[0], mods[2]
        if l2.in_features != l1.out_features or head.in_features != l2.out_features:
            raise ValueError("the policy path's layer shapes do not chain")
        live = [f for f in optimizer._flat if f["n"]]
        if len(live) != 1:
            raise ValueError("the optimizer must hold one flat parameter group")
        f = live[0]
        where = {id(p): off for p, (off, _, _) in zip(f["params"], f["views"])}

        def offset(p, name):
            if id(p) not in where:
                raise ValueError(f"{name} is not in the optimizer's flat bucket")
            return where[id(p)]

        offs = tuple(offset(p, name) for p, name in (
            (l1.weight, "the first trunk weight"), (l1.bias, "the first trunk bias"), (l2.weight, "the second trunk weight"),
            (l2.bias, "the second trunk bias"), (head.weight, "action_net.weight"), (head.bias, "action_net.bias")))
        ls = offset(policy.log_std, "log_std") if gaussian else -1
        layout = cls(int(l1.in_features), int(l1.out_features), int(l2.out_features), int(head.out_features), gaussian,
                     type(mods[1]) is nn.Tanh, offs, ls, int(f["flat"].numel()))
        layout.check()
        return layout

    def views(self, flat: th.Tensor):
        """``(W1, b1, W2, b2, W3, b3)`` as views of ``flat``."""
        shapes = [(self.H1, self.D), (self.H1,), (self.H2, self.H1), (self.H2,), (self.A, self.H2), (self.A,)]
        return [flat[off : off + k].view(shp) for off, k, shp in zip(self.offsets, self.sizes, shapes)]

    def log_std_view(self, flat: th.Tensor) -> Optional[th.Tensor]:
        return flat[self.log_std_offset : self.log_std_offset + self.A] if self.gaussian else None


def _check_call(ids: th.Tensor, flat: th.Tensor, layout: BCMlpLayout) -> None:
    layout.check()
    if ids.dim() != 2 or ids.dtype != th.int64:
        raise ValueError("ids must be int64 [G, B]")
    G, B = int(ids.shape[0]), int(ids.shape[1])
    if G < 1:
        raise ValueError("bc_mlp_steps needs at least one step (G >= 1)")
    if not 1 <= B <= MAX_BATCH:
        raise ValueError(f"bc_mlp_steps: a batch of {B} rows is outside 1..{MAX_BATCH}")
    if flat.numel() != layout.n:
        raise ValueError(f"the bucket has {flat.numel()} elements, the layout was made for {layout.n}")


def bc_mlp_reference(obs_src: th.Tensor, acts_src: th.Tensor, ids: th.Tensor, flat: th.Tensor, grad: Optional[th.Tensor],
                     exp_avg: th.Tensor, exp_avg_sq: th.Tensor, step: th.Tensor, layout: BCMlpLayout, lr: float,
                     betas=(0.9, 0.999), eps: float = 1e-8, ent_weight: float = 1e-3, l2_weight: float = 0.0,
                     keep_grad: bool = False, metrics: Optional[th.Tensor] = None) -> th.Tensor:
    """The ``G = ids.shape[0]`` minibatch steps in torch ops, in the dtype of ``flat``. Updates
    ``flat``, the moments and ``step`` in place; with ``keep_grad`` the last step's full gradient
    is left in ``grad`` (otherwise ``grad`` is not touched). Returns ``metrics [G, 7]``
    (``ops.rl.BC_METRICS`` order)."""
    _check_call(ids, flat, layout)
    G, B = int(ids.shape[0]), int(ids.shape[1])
    dt = flat.dtype
    if metrics is None:
        metrics = th.empty(G, len(BC_METRICS), dtype=dt, device=flat.device)
    group = {"betas": tuple(betas), "lr": lr, "eps": eps, "weight_decay": 0.0, "maximize": False,
             "decoupled_weight_decay": False}
    work = th.zeros_like(flat)  # the step's gradient (the bucket itself is only written with keep_grad)
    f = {"flat": flat, "grad": work, "m": exp_avg, "v": exp_avg_sq, "step": step}
    W1, b1, W2, b2, W3, b3 = layout.views(flat)
    gW1, gb1, gW2, gb2, gW3, gb3 = layout.views(work)
    log_std, g_log_std = layout.log_std_view(flat), layout.log_std_view(work)
    act = th.tanh if layout.tanh else th.relu
    dact = (lambda h: 1 - h * h) if layout.tanh else (lambda h: (h > 0).to(dt))
    n_rows = obs_src.shape[0]
    with th.no_grad():
        for g in range(G):
            rows = ids[g].clamp(0, n_rows - 1)
            x = obs_src[rows].reshape(B, -1).to(dt)
            h1 = act(x @ W1.T + b1)
            h2 = act(h1 @ W2.T + b2)
            out = h2 @ W3.T + b3
            if layout.gaussian:
                a = acts_src[rows].reshape(B, -1).to(dt)
                std = th.exp(log_std)
                z = (a - out) / std
                logp = (-0.5 * z * z - log_std - _HALF_LOG_2PI).sum(1)
                entropy = (0.5 + _HALF_LOG_2PI + log_std).sum()  # the same for every row
                dout = -(z / std) / B
                g_log_std.copy_((1 - z * z).sum(0) / B - ent_weight)
            else:
                a = acts_src[rows].reshape(B).long().clamp(0, layout.A - 1)
                logits = out - out.logsumexp(dim=1, keepdim=True)
                p = logits.exp()
                ent_rows = -(p * logits).sum(1)
                logp = logits.gather(1, a.reshape(B, 1)).squeeze(1)
                entropy = ent_rows.mean()
                onehot = th.zeros_like(p).scatter_(1, a.reshape(B, 1), 1.0)
                dout = ((p - onehot) + ent_weight * (p * (logits + ent_rows.reshape(B, 1)))) / B
            dz2 = (dout @ W3) * dact(h2)
            dz1 = (dz2 @ W2) * dact(h1)
            gW3.copy_(dout.T @ h2)
            gb3.copy_(dout.sum(0))
            gW2.copy_(dz2.T @ h1)
            gb2.copy_(dz2.sum(0))
            gW1.copy_(dz1.T @ x)
            gb1.copy_(dz1.sum(0))
            work.add_(flat, alpha=l2_weight)
            neglogp = -logp.mean()
            ent_loss = -ent_weight * entropy
            l2_norm = flat.square().sum() / 2
            l2_loss = l2_weight * l2_norm
            metrics[g] = th.stack([neglogp, entropy, ent_loss, logp.exp().mean(), l2_norm, l2_loss,
                                   neglogp + ent_loss + l2_loss])
            if keep_grad and g == G - 1:
                grad.copy_(work)
            step.add_(1.0)
            FusedAdam._step_reference(group, f)  # (clears the work gradient it consumed)
    return metrics


def bc_mlp_steps(obs_src: th.Tensor, acts_src: th.Tensor, ids: th.Tensor, flat: th.Tensor, grad: Optional[th.Tensor],
                 exp_avg: th.Tensor, exp_avg_sq: th.Tensor, step: th.Tensor, layout: BCMlpLayout, lr: float,
                 betas=(0.9, 0.999), eps: float = 1e-8, ent_weight: float = 1e-3, l2_weight: float = 0.0,
                 keep_grad: bool = False, metrics: Optional[th.Tensor] = None) -> th.Tensor:
    """``G = ids.shape[0]`` BC minibatch steps on the flat buckets: ONE kernel launch for GPU
    tensors, :func:`bc_mlp_reference` for CPU tensors. ``ids [G, B]`` are flat row ids into
    ``obs_src [N, D]`` fp32 and ``acts_src`` (``[N]`` int64 for a categorical head, ``[N, A]`` fp32
    for a Gaussian one). With ``keep_grad`` the last step's full gradient is left in ``grad``;
    without it ``grad`` is neither read nor written. Returns ``metrics [G, 7]``."""
    if not ops.use_kernel(flat):
        return bc_mlp_reference(obs_src, acts_src, ids, flat, grad, exp_avg, exp_avg_sq, step, layout, lr, betas, eps,
                                ent_weight, l2_weight, keep_grad, metrics)
    if keep_grad and grad is None:
        raise ValueError("keep_grad needs the gradient bucket")
    if metrics is None:
        metrics = th.empty(int(ids.shape[0]), len(BC_METRICS), dtype=flat.dtype, device=flat.device)
    ops.native().bc_mlp_steps(obs_src, acts_src, ids, flat, grad if keep_grad else None, exp_avg, exp_avg_sq, step,
                              list(layout.offsets), int(layout.log_std_offset), layout.D, layout.H1, layout.H2, layout.A,
                              bool(layout.gaussian), bool(layout.tanh), float(lr), float(betas[0]), float(betas[1]),
                              float(eps), float(ent_weight), float(l2_weight), metrics)
    return metrics
