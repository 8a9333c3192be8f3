"""Plain PyTorch float64 reference of one fused GAIL discriminator update.

The numerics reference for ``DiscPlan`` (csrc/kernels/disc.hip, the discriminator instance
of csrc/kernels/tmlp.hip): ``AdversarialTrainer.train_disc`` for a ``BasicRewardNet`` with
given row indices. Per minibatch ``k`` of ``minibatch`` expert and ``minibatch`` generator rows:

* gather ``[expert rows ; generator rows]`` into ``obs | act or one-hot | next_obs | done``;
* two-pass batch mean / biased variance, Chan-merged into the reward net's RunningNorm, and
  its first ``obs_dim`` columns into the policy's RunningNorm (the side effect of GAIL's
  log-prob pass);
* normalise with the *merged* state, run the MLP, BCE-with-logits against labels 1 (expert)
  / 0 (generator), scaled by ``minibatch / batch``; gradients accumulate over minibatches.

After the last minibatch: ``torch.optim.Adam``'s update (coupled ``weight_decay``) and the
statistics sums of the last minibatch only. Everything is written out by hand (forward,
backward, Adam) on CPU float64 tensors; no project kernel or op is used.

``bf16_operands=True`` rounds every matrix-product operand (activations, weights, dZ) to
bfloat16 first, as the MFMA kernels do. It is there to size test tolerances, not as a reference.
"""

from __future__ import annotations

from typing import Dict, List, Mapping, Optional, Sequence

import torch as th

F64 = th.float64


def gather_rows(src: Mapping[str, th.Tensor], idx: th.Tensor, layout: Mapping[str, int]) -> th.Tensor:
    """Rows ``idx`` of one source set in the reward-net input layout (float64)."""
    cols = []
    if layout["use_state"]:
        cols.append(src["obs"][idx].to(F64))
    if layout["use_action"]:
        if layout["act_discrete"]:
            a = src["acts"].reshape(-1)[idx]
            cols.append((a[:, None] == th.arange(layout["act_width"])[None, :]).to(F64))
        else:
            cols.append(src["acts"][idx].to(F64))
    if layout["use_next_state"]:
        cols.append(src["next_obs"][idx].to(F64))
    if layout["use_done"]:
        cols.append(src["dones"][idx].to(F64)[:, None])
    return th.cat(cols, 1)


def batch_moments(x: th.Tensor):
    """Two-pass mean and biased variance over dim 0."""
    mean = x.mean(0)
    return mean, ((x - mean) ** 2).mean(0)


def chan_merge(state: Mapping[str, th.Tensor], bmean: th.Tensor, bvar: th.Tensor, n: int) -> Dict[str, th.Tensor]:
    """``RunningNorm.update_stats``: merge batch moments of ``n`` rows into ``state``."""
    count = int(state["count"])
    tot = count + n
    delta = bmean - state["mean"]
    mean = state["mean"] + delta * n / tot
    var = (state["var"] * count + bvar * n + delta**2 * count * n / tot) / tot
    return {"mean": mean, "var": var, "count": tot}


def norm_state(s: Optional[Mapping]) -> Optional[Dict[str, th.Tensor]]:
    """A running norm's ``mean, var, count`` as float64 CPU copies."""
    if s is None:
        return None
    return {"mean": s["mean"].detach().cpu().to(F64).clone(), "var": s["var"].detach().cpu().to(F64).clone(),
            "count": int(s["count"])}


def _bf16(t: th.Tensor) -> th.Tensor:
    return t.to(th.float32).to(th.bfloat16).to(F64)


def _act(name: str, z: th.Tensor) -> th.Tensor:
    if name == "relu":
        return z.clamp_min(0)
    if name == "tanh":
        return th.tanh(z)
    raise ValueError(name)


def _act_grad_from_out(name: str, h: th.Tensor) -> th.Tensor:
    if name == "relu":
        return (h > 0).to(F64)
    return 1 - h * h


def disc_update_reference(*, expert: Mapping[str, th.Tensor], gen: Mapping[str, th.Tensor], e_idx: th.Tensor,
                          g_idx: th.Tensor, layout: Mapping[str, int], batch: int, minibatch: int,
                          Ws: Sequence[th.Tensor], bs: Sequence[th.Tensor], hidden_act: str,
                          rew_norm: Optional[Mapping], pol_norm: Optional[Mapping], rew_eps: float,
                          adam: Mapping, merge_rew: bool = True, merge_pol: bool = True,
                          bf16_operands: bool = False) -> Dict:
    """One discriminator update.

    ``expert`` / ``gen``: ``obs``, ``acts`` (int64 indices when ``layout['act_discrete']``),
    ``next_obs``, ``dones``. ``layout``: ``obs_dim, act_width, use_state, use_action,
    use_next_state, use_done, act_discrete``. ``rew_norm`` / ``pol_norm``: ``mean, var, count``
    or None. ``adam``: ``exp_avg, exp_avg_sq`` (flat), ``step`` (steps already taken), ``lr,
    beta1, beta2, eps, weight_decay``.

    Returns ``X``, ``rew_states``, ``pol_states``, ``logits``, ``preacts`` (the hidden
    layers' pre-activations) with one entry per minibatch,
    ``grads`` (flat ``W0, b0, W1, b1, ...``), ``stats`` (sums over the last minibatch: BCE,
    correct, predicted generator, expert correct, generator correct, entropy) and ``params``,
    ``exp_avg``, ``exp_avg_sq`` after Adam."""
    rd = _bf16 if bf16_operands else (lambda t: t)
    e_idx, g_idx = e_idx.cpu().long(), g_idx.cpu().long()
    expert = {k: v.detach().cpu() for k, v in expert.items()}
    gen = {k: v.detach().cpu() for k, v in gen.items()}
    Ws = [w.detach().cpu().to(F64) for w in Ws]
    bs = [b.detach().cpu().to(F64) for b in bs]
    L = len(Ws)
    rew, pol = norm_state(rew_norm), norm_state(pol_norm)
    mb, n = minibatch, 2 * minibatch
    assert batch % mb == 0
    y = th.cat([th.ones(mb, dtype=F64), th.zeros(mb, dtype=F64)])
    gW = [th.zeros_like(w) for w in Ws]
    gb = [th.zeros_like(b) for b in bs]
    out: Dict[str, List] = {"X": [], "rew_states": [], "pol_states": [], "logits": [], "preacts": []}
    for k in range(batch // mb):
        sl = slice(k * mb, (k + 1) * mb)
        X = th.cat([gather_rows(expert, e_idx[sl], layout), gather_rows(gen, g_idx[sl], layout)])
        bmean, bvar = batch_moments(X)
        if rew is not None and merge_rew:
            rew = chan_merge(rew, bmean, bvar, n)
        if pol is not None and merge_pol and layout["use_state"]:
            D = layout["obs_dim"]
            pol = chan_merge(pol, bmean[:D], bvar[:D], n)
        out["X"].append(X)
        out["rew_states"].append(None if rew is None else dict(rew))
        out["pol_states"].append(None if pol is None else dict(pol))
        h = X if rew is None else (X - rew["mean"]) / th.sqrt(rew["var"] + rew_eps)
        # forward, every layer input kept (rounded as the product sees it)
        hs, zs = [], []
        for l in range(L):
            h = rd(h)
            hs.append(h)
            z = h @ rd(Ws[l]).T + bs[l]
            zs.append(z)
            h = z if l == L - 1 else _act(hidden_act, z)
        z = z.reshape(-1)
        out["logits"].append(z)
        out["preacts"].append(zs[:-1])
        # d(mean BCE * mb / batch) / dz
        dz = ((th.sigmoid(z) - y) * (mb / batch / n))[:, None]
        for l in range(L - 1, -1, -1):
            gb[l] += dz.sum(0)
            gW[l] += rd(dz).T @ hs[l]
            if l > 0:
                dz = (rd(dz) @ rd(Ws[l])) * _act_grad_from_out(hidden_act, hs[l])
    sp = th.nn.functional.softplus(z)
    sg = th.sigmoid(z)
    gen_pred, gen_true = z < 0, y == 0
    correct = gen_pred == gen_true
    out["stats"] = th.stack([(sp - z * y).sum(), correct.sum().to(F64), gen_pred.sum().to(F64),
                             (~gen_true & correct).sum().to(F64), (gen_true & correct).sum().to(F64),
                             (sp - z * sg).sum()])
    grads = th.cat([t.reshape(-1) for pair in zip(gW, gb) for t in pair])
    params = th.cat([t.reshape(-1) for pair in zip(Ws, bs) for t in pair])
    out["grads"] = grads
    p, m, v = adam_step_reference(params, grads, adam["exp_avg"], adam["exp_avg_sq"], int(adam["step"]) + 1,
                                  adam["lr"], adam["beta1"], adam["beta2"], adam["eps"], adam["weight_decay"])
    out["params"], out["exp_avg"], out["exp_avg_sq"] = p, m, v
    return out


def adam_step_reference(params, grads, exp_avg, exp_avg_sq, t: int, lr, beta1, beta2, eps, weight_decay):
    """``torch.optim.Adam`` step number ``t`` (1-based) on flat float64 tensors."""
    p, g = params.detach().cpu().to(F64), grads.detach().cpu().to(F64)
    m, v = exp_avg.detach().cpu().to(F64), exp_avg_sq.detach().cpu().to(F64)
    if weight_decay != 0:
        g = g + weight_decay * p
    m = beta1 * m + (1 - beta1) * g
    v = beta2 * v + (1 - beta2) * g * g
    denom = v.sqrt() / (1 - beta2**t) ** 0.5 + eps
    return p - lr / (1 - beta1**t) * m / denom, m, v
