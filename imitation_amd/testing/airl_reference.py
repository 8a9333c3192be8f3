"""Plain PyTorch float64 reference of one fused AIRL discriminator update.

The numerics reference for ``AirlDiscPlan`` (csrc/kernels/airl_disc.hip, the MLP blocks of
csrc/include/ia/dmlp.h, the Adam step of csrc/kernels/disc.hip):
``AdversarialTrainer.train_disc`` with AIRL's logits and a shaped reward net, for given row
indices. Per minibatch ``k`` of ``minibatch`` expert and ``minibatch`` generator rows:

* gather ``[expert rows ; generator rows]``: the base net's input ``X`` in the layout
  ``obs | act or one-hot | next_obs | done``, the observations ``S``, the next observations
  ``S2``, the stored actions and the done flags;
* two-pass batch mean / biased variance of ``X``, of ``S2`` and of ``S``; Chan merges in the
  order base norm (``X``), potential norm (``S2``), potential norm (``S``), policy norm (``S``);
* every forward normalises with the state as merged at that point: ``Phi(s')`` with the
  potential state after its first merge, ``Phi(s)`` with the state after its second;
* ``log pi(a|s)`` of the policy under no_grad: diagonal Gaussian (``log_std``, the raw stored
  actions) or categorical (log-softmax at the action index);
* ``logit = r + gamma (1 - d) Phi(s') - Phi(s) - log pi``, BCE against labels 1 (expert) /
  0 (generator), scaled by ``minibatch / batch``; backward into the base net and into both
  potential passes; gradients accumulate over minibatches in the flat order base
  ``W0, b0, ...`` then potential.

After the last minibatch: ``torch.optim.Adam``'s update and the statistics sums of the last
minibatch only. Everything is written out by hand on CPU float64 tensors; no project kernel
or op is used.

``bf16_operands=True`` rounds every matrix-product operand (normalised inputs, hidden
activations, weights, dZ; all three nets, both directions) to bfloat16 first, as the MFMA
kernels do. It is there to size test tolerances, not as a reference.
"""

from __future__ import annotations

import math
from typing import Dict, List, Mapping, Optional

import torch as th

from imitation_amd.testing.disc_reference import (F64, _act, _act_grad_from_out, _bf16, adam_step_reference,
                                                  batch_moments, chan_merge, gather_rows, norm_state)

_HALF_LOG_2PI = 0.5 * math.log(2.0 * math.pi)


def _net64(net: Mapping) -> Dict:
    return dict(Ws=[w.detach().cpu().to(F64) for w in net["Ws"]], bs=[b.detach().cpu().to(F64) for b in net["bs"]],
                act=net["act"])


def _normalise(x: th.Tensor, state: Optional[Mapping], eps: float) -> th.Tensor:
    return x if state is None else (x - state["mean"]) / th.sqrt(state["var"] + eps)


def _forward(net: Mapping, x: th.Tensor, rd):
    """Outputs of the (identity) last layer, every layer's input as the product sees it, and
    the hidden layers' pre-activations."""
    L = len(net["Ws"])
    h, hs, zs = x, [], []
    for l in range(L):
        h = rd(h)
        hs.append(h)
        z = h @ rd(net["Ws"][l]).T + net["bs"][l]
        zs.append(z)
        h = z if l == L - 1 else _act(net["act"], z)
    return z, hs, zs[:-1]


def _backward(net: Mapping, hs: List[th.Tensor], dy: th.Tensor, gW: List[th.Tensor], gb: List[th.Tensor], rd) -> None:
    """Adds dW / db for per-row output gradients ``dy`` ([rows]) to ``gW`` / ``gb``."""
    dz = dy[:, None]
    for l in range(len(net["Ws"]) - 1, -1, -1):
        gb[l] += dz.sum(0)
        gW[l] += rd(dz).T @ hs[l]
        if l > 0:
            dz = (rd(dz) @ rd(net["Ws"][l])) * _act_grad_from_out(net["act"], hs[l])


def airl_update_reference(*, expert: Mapping[str, th.Tensor], gen: Mapping[str, th.Tensor], e_idx: th.Tensor,
                          g_idx: th.Tensor, layout: Mapping[str, int], batch: int, minibatch: int, base: Mapping,
                          pot: Mapping, pol: Mapping, log_std: Optional[th.Tensor], gamma: float,
                          b_norm: Optional[Mapping], p_norm: Optional[Mapping], q_norm: Optional[Mapping],
                          eps_b: float, eps_p: float, eps_q: float, adam: Mapping, merge_b: bool = True,
                          merge_p: bool = True, merge_q: bool = True, bf16_operands: bool = False) -> Dict:
    """One AIRL discriminator update.

    ``expert`` / ``gen``: ``obs``, ``acts`` (int64 indices when ``layout['act_discrete']``),
    ``next_obs``, ``dones``. ``layout``: as ``disc_reference.gather_rows`` takes it (the base
    net's input). ``base`` / ``pot`` / ``pol``: ``Ws``, ``bs``, ``act`` (the policy's last layer
    is its action head). ``b_norm`` / ``p_norm`` / ``q_norm``: ``mean, var, count`` of the base,
    potential and policy running norms, or None. ``adam``: as ``disc_update_reference``.

    Returns, with one entry per minibatch: ``X``, ``S``, ``S2``, ``Act``, ``Done`` (gathered),
    ``b_states``, ``p_states_next`` (potential norm after the ``s'`` merge), ``p_states`` (after
    the ``s`` merge), ``q_states``, ``logp``, ``r``, ``phi_next``, ``phi``, ``logits`` and
    ``preacts`` (dict of the hidden pre-activations of ``base``, ``pot_next``, ``pot``). And
    ``grads`` (flat), ``stats`` (sums over the last minibatch: BCE, correct, predicted
    generator, expert correct, generator correct, entropy), ``params``, ``exp_avg``,
    ``exp_avg_sq`` after Adam."""
    rd = _bf16 if bf16_operands else (lambda t: t)
    e_idx, g_idx = e_idx.cpu().long(), g_idx.cpu().long()
    expert = {k: v.detach().cpu() for k, v in expert.items()}
    gen = {k: v.detach().cpu() for k, v in gen.items()}
    base, pot, pol = _net64(base), _net64(pot), _net64(pol)
    discrete = bool(layout["act_discrete"])
    if not discrete:
        log_std = log_std.detach().cpu().to(F64)
    bst, pst, qst = norm_state(b_norm), norm_state(p_norm), norm_state(q_norm)
    mb, n = minibatch, 2 * minibatch
    assert batch % mb == 0
    y = th.cat([th.ones(mb, dtype=F64), th.zeros(mb, dtype=F64)])
    g = {q: ([th.zeros_like(w) for w in net["Ws"]], [th.zeros_like(b) for b in net["bs"]])
         for q, net in (("base", base), ("pot", pot))}
    keys = ("X", "S", "S2", "Act", "Done", "b_states", "p_states_next", "p_states", "q_states", "logp", "r", "phi_next",
            "phi", "logits", "preacts")
    out: Dict[str, List] = {k: [] for k in keys}

    def both(key, f=lambda t: t.to(F64)):
        return th.cat([f(expert[key][e_idx[sl]]), f(gen[key][g_idx[sl]])])

    for k in range(batch // mb):
        sl = slice(k * mb, (k + 1) * mb)
        X = th.cat([gather_rows(expert, e_idx[sl], layout), gather_rows(gen, g_idx[sl], layout)])
        S, S2, d = both("obs"), both("next_obs"), both("dones")
        acts = both("acts", lambda t: t.reshape(t.shape[0], -1)) if discrete else both("acts")
        # merges, in the kernel's (and the host path's) order
        if bst is not None and merge_b:
            bst = chan_merge(bst, *batch_moments(X), n)
        p_next = pst
        if pst is not None and merge_p:
            p_next = chan_merge(pst, *batch_moments(S2), n)
            pst = chan_merge(p_next, *batch_moments(S), n)
        if qst is not None and merge_q:
            qst = chan_merge(qst, *batch_moments(S), n)
        # log pi(a|s), no gradient
        heads, _, _ = _forward(pol, _normalise(S, qst, eps_q), rd)
        if discrete:
            logp = (heads - heads.logsumexp(1, keepdim=True)).gather(1, acts.long()).reshape(-1)
        else:
            zz = (acts - heads) * th.exp(-log_std)
            logp = (-0.5 * zz * zz - log_std - _HALF_LOG_2PI).sum(1)
        r, hs_b, zs_b = _forward(base, _normalise(X, bst, eps_b), rd)
        phi_next, hs_n, zs_n = _forward(pot, _normalise(S2, p_next, eps_p), rd)
        phi, hs_p, zs_p = _forward(pot, _normalise(S, pst, eps_p), rd)
        r, phi_next, phi = r.reshape(-1), phi_next.reshape(-1), phi.reshape(-1)
        z = r + gamma * (1 - d) * phi_next - phi - logp
        for key, val in zip(keys, (X, S, S2, acts.to(F64), d, bst, p_next, pst, qst, logp, r, phi_next, phi, z,
                                   dict(base=zs_b, pot_next=zs_n, pot=zs_p))):
            out[key].append(dict(val) if key.endswith("states") and val is not None else val)
        # d(mean BCE * mb / batch) / dlogit, then into the three passes
        dl = (th.sigmoid(z) - y) * (mb / batch / n)
        _backward(base, hs_b, dl, *g["base"], rd)
        _backward(pot, hs_n, gamma * (1 - d) * dl, *g["pot"], rd)
        _backward(pot, hs_p, -dl, *g["pot"], rd)
    sp = th.nn.functional.softplus(z)
    sg = th.sigmoid(z)
    gen_pred, gen_true = z < 0, y == 0
    correct = gen_pred == gen_true
    out["stats"] = th.stack([(sp - z * y).sum(), correct.sum().to(F64), gen_pred.sum().to(F64),
                             (~gen_true & correct).sum().to(F64), (gen_true & correct).sum().to(F64),
                             (sp - z * sg).sum()])
    flat = lambda Ws, bs: [t.reshape(-1) for pair in zip(Ws, bs) for t in pair]  # noqa: E731
    grads = th.cat(flat(*g["base"]) + flat(*g["pot"]))
    params = th.cat(flat(base["Ws"], base["bs"]) + flat(pot["Ws"], pot["bs"]))
    out["grads"] = grads
    p, m, v = adam_step_reference(params, grads, adam["exp_avg"], adam["exp_avg_sq"], int(adam["step"]) + 1,
                                  adam["lr"], adam["beta1"], adam["beta2"], adam["eps"], adam["weight_decay"])
    out["params"], out["exp_avg"], out["exp_avg_sq"] = p, m, v
    return out
