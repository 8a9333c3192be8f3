"""The fused SAC update (``imitation_amd.ops.sac``; ``csrc/kernels/sac_update.hip``).

CPU part: ``sac_update_reference`` is the maths of the eager ``SAC.train`` step, the cases keep
their margins from the branch points, and every eligibility rule of ``SAC`` keeps the eager step
with its own reason. GPU part: the kernel against an fp64 evaluation, its Adam hand-off,
multi-step launches, determinism, the target bucket views and the launcher's limits."""

import functools
import itertools

import numpy as np
import pytest
import torch as th
from torch import nn
from torch.nn import functional as F

from imitation_amd.ops import sac as su

GAMMA, TAU = 0.99, 0.05
LR = 1e-3
HP = (LR, 0.9, 0.999, 1e-8)
FIXED_ENT_COEF = 0.2
G_MAX = 3  # every case draws the ids and the noise of three steps; a run uses the first G
VARIANTS = ("base", "done1", "timeout", "fixed", "clamp", "squash")
# name -> (D, A, actor [H1, H2], critic [H1, H2], n_a, n_e, rows_a, valid_a, rows_e): valid_a < rows_a is a ring
# that is not full yet
SHAPES = {
    "p": (3, 1, (24, 40), (24, 40), 2, 3, 24, 12, 7),        # Pendulum; ring half filled, a duplicate id
    "h": (17, 6, (64, 64), (64, 64), 128, 128, 300, 300, 200),  # HalfCheetah / SQIL: four full chunks
    "e": (58, 6, (64, 64), (48, 64), 110, 110, 300, 300, 150),  # D + A = 64, ragged last chunk
    "e1": (58, 6, (64, 64), (48, 64), 220, 0, 300, 300, 0),   # one source
    "o": (1, 1, (1, 1), (1, 1), 1, 0, 3, 3, 0),
}
# ("o", "clamp") is no case: its one log_std element per forward cannot be clamped on both sides
# with half of the elements unclamped, which the clamp variant is defined by
GRID = [(s, v) for s, v in itertools.product(SHAPES, VARIANTS) if (s, v) != ("o", "clamp")]
# The seed of every case: the first of 0, 1, 2, ... at which the case's fp64 evaluation keeps the
# branch margins over all three steps and, at the larger shapes, has rows on both sides of
# min(Q1, Q2) (test_cases_keep_their_branch_margins); "tui2": shape h with target_update_interval = 2
SEEDS = {
    ("p", "base"): 0, ("p", "done1"): 1, ("p", "timeout"): 0, ("p", "fixed"): 0, ("p", "clamp"): 92, ("p", "squash"): 0,
    ("h", "base"): 10, ("h", "done1"): 10, ("h", "timeout"): 10, ("h", "fixed"): 2, ("h", "clamp"): 26, ("h", "squash"): 10,
    ("e", "base"): 15, ("e", "done1"): 4, ("e", "timeout"): 7, ("e", "fixed"): 7, ("e", "clamp"): 7, ("e", "squash"): 7,
    ("e1", "base"): 17, ("e1", "done1"): 27, ("e1", "timeout"): 27, ("e1", "fixed"): 4, ("e1", "clamp"): 4, ("e1", "squash"): 7,
    ("o", "base"): 0, ("o", "done1"): 0, ("o", "timeout"): 0, ("o", "fixed"): 0, ("o", "squash"): 0,
    "tui2": 10,
}
MARGIN = 1e-3


def _init(views, gen):
    for v in views:  # nn.Linear's default range
        k = v.shape[-1] if v.dim() == 2 else None
        v.copy_((th.rand(v.shape, generator=gen) * 2 - 1) / np.sqrt(k if k else max(v.numel(), 1)))


def _source(gen, rows, valid, D, A, variant):
    obs, nxt = th.randn(rows, D, generator=gen), th.randn(rows, D, generator=gen)
    act = th.rand(rows, A, generator=gen) * 2 - 1
    rew = th.randn(rows, generator=gen)
    done = th.ones(rows) if variant == "done1" else (th.rand(rows, generator=gen) < 0.3).float()
    tmo = th.zeros(rows)
    if variant == "timeout":  # every other row ended by a time limit: done, but bootstrapped
        done[::2] = 1.0
        tmo[::2] = 1.0
    for t in (obs, nxt, act, rew):  # rows the ring has not filled must never be read
        t[valid:] = float("nan")
    return [obs, nxt, act, rew, done, tmo]


def _bucket(n):
    n4 = n + (-n) % 4
    return dict(flat=th.zeros(n4), grad=th.zeros(n4), m=th.zeros(n4), v=th.zeros(n4), step=th.zeros(1))


def build_case(shape, variant, seed):
    D, A, a_arch, c_arch, n_a, n_e, rows_a, valid_a, rows_e = SHAPES[shape]
    gen = th.Generator().manual_seed(seed)
    L = su.SACLayout.from_dims(D, A, a_arch, c_arch)
    actor, critic = _bucket(L.n_actor), _bucket(L.n_critic)
    target = th.zeros_like(critic["flat"])
    _init(L.actor_views(actor["flat"]), gen)
    for buf in (critic["flat"], target):
        for cv in L.critic_views(buf):
            _init(cv, gen)
            cv[4].mul_(4.0)  # spread the Q-values: min(Q1, Q2) is a branch point the rows must keep away from
            cv[5].mul_(4.0)
    av = L.actor_views(actor["flat"])
    if variant == "clamp":  # log_std pre-activations on both sides of [-20, 2]
        av[6].mul_(60.0)
        av[7].mul_(20.0).sub_(9.0)
    if variant == "squash":  # large means: |a| -> 1
        av[4].mul_(12.0)
        av[5].mul_(4.0)
    ent = None
    if variant != "fixed":
        ent = _bucket(1)
        ent["flat"][0] = float(np.log(0.7))
    src_a = _source(gen, rows_a, valid_a, D, A, variant)
    src_b = _source(gen, rows_e, rows_e, D, A, variant) if n_e else None
    if src_b is not None:
        src_b[3] = th.ones(rows_e)  # SQIL: expert reward 1
        src_a[3] = th.where(th.isnan(src_a[3]), src_a[3], th.zeros(rows_a))
    ids_a = th.randint(0, valid_a, (G_MAX, n_a), generator=gen)
    if n_a > 1:
        ids_a[:, 1] = ids_a[:, 0]  # a duplicate row in every batch
    ids_b = th.randint(0, rows_e, (G_MAX, n_e), generator=gen) if n_e else None
    B = n_a + n_e
    eps_pi, eps_next = th.randn(G_MAX, B, A, generator=gen), th.randn(G_MAX, B, A, generator=gen)
    return dict(L=L, src_a=src_a, src_b=src_b, ids_a=ids_a, ids_b=ids_b, eps_pi=eps_pi, eps_next=eps_next,
                state=dict(actor=actor, critic=critic, ent=ent, target=target), variant=variant)


def clone_state(state, dtype=None, device=None):
    def mv(t):
        t = t.clone() if dtype is None else t.to(dtype)
        return t if device is None else t.to(device)

    return {k: None if v is None else (mv(v) if isinstance(v, th.Tensor) else {kk: mv(t) for kk, t in v.items()})
            for k, v in state.items()}


def cast_src(src, dtype, device=None):
    if src is None:
        return None
    return [t.to(dtype) if device is None else t.to(dtype).to(device) for t in src]


def run(fn, case, state, G=1, lo=0, hp=HP, tui=1, dtype=th.float32, device=None, **kw):
    """Steps lo .. lo + G of the case on ``state`` (in place)."""
    dev = lambda t: None if t is None else (t if device is None else t.to(device))  # noqa: E731
    ids_b = None if case["ids_b"] is None else dev(case["ids_b"][lo : lo + G].contiguous())
    return fn(cast_src(case["src_a"], dtype, device), cast_src(case["src_b"], dtype, device),
              dev(case["ids_a"][lo : lo + G].contiguous()), ids_b, dev(case["eps_pi"][lo : lo + G].to(dtype).contiguous()),
              dev(case["eps_next"][lo : lo + G].to(dtype).contiguous()), state["actor"], state["critic"], state["ent"],
              state["target"], case["L"], actor_hp=hp, critic_hp=hp, ent_hp=hp, ent_coef=FIXED_ENT_COEF,
              target_entropy=-float(case["L"].A), gamma=GAMMA, tau=TAU, target_update_interval=tui, **kw)


def margins(case, tui=1):
    """The case's distances from its branch points over all G_MAX steps, on the fp64 evaluation:
    (min |Q1 - Q2| over the rows at a_pi and at a', min distance of a log_std pre-activation from
    -20 and 2, numbers of elements clamped below / above / not at all)."""
    info = []
    run(su.sac_update_reference, case, clone_state(case["state"], th.float64), G=G_MAX, tui=tui, dtype=th.float64, info=info)
    qgap = min(float((i[k][:, 0] - i[k][:, 1]).abs().min()) for i in info for k in ("q_pi", "q_next"))
    raw = th.cat([i[k].reshape(-1) for i in info for k in ("raw", "raw_next")])
    edge = float(th.minimum((raw - su.LOG_STD_MIN).abs(), (raw - su.LOG_STD_MAX).abs()).min())
    both = any(float((i["q_pi"][:, 0] < i["q_pi"][:, 1]).float().mean()) not in (0.0, 1.0) for i in info)
    return qgap, edge, int((raw < su.LOG_STD_MIN).sum()), int((raw > su.LOG_STD_MAX).sum()), raw.numel(), both


@functools.lru_cache(maxsize=None)
def make_case(shape, variant, tui=1):
    """The case at its seed, built once and shared; nothing changes it (every run works on clones)."""
    return build_case(shape, variant, SEEDS["tui2" if tui == 2 else (shape, variant)])


# ------------------------------------------------------------------------------------ CPU
@pytest.mark.parametrize("shape,variant", GRID + [("h", "tui2")])
def test_cases_keep_their_branch_margins(shape, variant):
    """A condition on the inputs, not a tolerance: min(Q1, Q2) and the log_std clamp are branch
    points, so every row's |Q1 - Q2| (at a_pi and at a') and every log_std pre-activation's
    distance from -20 and 2 is at least 1e-3 on the fp64 evaluation, over all three steps; the
    clamp variant has elements clamped on both sides and at least half unclamped."""
    tui = 2 if variant == "tui2" else 1
    case = make_case(shape, "base" if variant == "tui2" else variant, tui)
    qgap, edge, lo, hi, n, both = margins(case, tui)
    print(f"sac case {shape} {variant}: min |Q1 - Q2| {qgap:.3e}, log_std edge distance {edge:.3e}, clamped {lo} below "
          f"{hi} above of {n}, both critics selected: {both}")
    assert qgap >= MARGIN and edge >= MARGIN
    if variant == "clamp":
        assert lo >= 1 and hi >= 1 and 2 * (lo + hi) <= n
    if shape in ("h", "e", "e1"):
        assert both, "min(Q1, Q2) must select each critic for some row"


def _modules(case):
    L = case["L"]
    st = case["state"]

    def fill(mods, views):
        for m in mods:
            m.double()
        with th.no_grad():
            for p, v in zip([p for m in mods for p in m.parameters()], views):
                p.copy_(v)

    def critic_nets(flat):
        nets = [nn.Sequential(nn.Linear(L.D + L.A, L.critic_arch[0]), nn.ReLU(), nn.Linear(*L.critic_arch), nn.ReLU(),
                              nn.Linear(L.critic_arch[1], 1)) for _ in range(2)]
        fill(nets, [v for cv in L.critic_views(flat) for v in cv])
        return nets

    trunk = nn.Sequential(nn.Linear(L.D, L.actor_arch[0]), nn.ReLU(), nn.Linear(*L.actor_arch), nn.ReLU())
    mu, log_std = nn.Linear(L.actor_arch[1], L.A), nn.Linear(L.actor_arch[1], L.A)
    fill([trunk, mu, log_std], L.actor_views(st["actor"]["flat"]))
    return (trunk, mu, log_std), critic_nets(st["critic"]["flat"]), critic_nets(st["target"])


def as_double(case):
    cast = lambda t: t.double() if isinstance(t, th.Tensor) and t.is_floating_point() else t  # noqa: E731
    out = {k: [cast(t) for t in v] if isinstance(v, list) else cast(v) for k, v in case.items()}
    out["state"] = clone_state(case["state"], th.float64)
    return out


def _eager_steps(case, G, tui):
    """``SAC.train``'s gradient step (rl/sac.py) on fp64 torch modules holding the case's weights,
    with ``th.optim.Adam``, the case's row ids and its noise in place of the actor's draws.
    ``case``: :func:`as_double`'s."""
    from imitation_amd.rl.distributions import SquashedDiagGaussianDistribution
    from imitation_amd.rl.off_policy import polyak_update

    L, st = case["L"], case["state"]
    (trunk, mu, log_std), critics, targets = _modules(case)
    actor_params = [p for m in (trunk, mu, log_std) for p in m.parameters()]
    critic_params = [p for m in critics for p in m.parameters()]
    target_params = [p for m in targets for p in m.parameters()]
    opt_a, opt_c = th.optim.Adam(actor_params, lr=LR), th.optim.Adam(critic_params, lr=LR)
    log_ent, opt_e = None, None
    if st["ent"] is not None:
        log_ent = st["ent"]["flat"][:1].clone().requires_grad_(True)
        opt_e = th.optim.Adam([log_ent], lr=LR)
    dist = SquashedDiagGaussianDistribution(L.A)
    target_entropy = -float(L.A)

    def action_log_prob(obs, eps):
        latent = trunk(obs)
        mean = mu(latent)
        ls = th.clamp(log_std(latent), su.LOG_STD_MIN, su.LOG_STD_MAX)
        dist.proba_distribution(mean, ls)
        dist.gaussian_actions = mean + th.exp(ls) * eps  # DiagGaussianDistribution.sample with the given noise
        act = th.tanh(dist.gaussian_actions)
        return act, dist.log_prob(act, dist.gaussian_actions)

    out = dict(critic_loss=[], actor_loss=[], ent_coef=[], ent_coef_loss=[], actor_grads=[], critic_grads=[], ent_grads=[])
    for g in range(G):
        parts = [[t[case["ids_a"][g]] for t in case["src_a"]]]
        if case["src_b"] is not None:
            parts.append([t[case["ids_b"][g]] for t in case["src_b"]])
        obs, nxt, act, rew, done, tmo = (th.cat([p[i] for p in parts]) for i in range(6))
        dones, rew = (done * (1 - tmo)).reshape(-1, 1), rew.reshape(-1, 1)
        actions_pi, log_prob = action_log_prob(obs, case["eps_pi"][g])
        log_prob = log_prob.reshape(-1, 1)
        if opt_e is not None:
            ent_coef = th.exp(log_ent.detach())
            ent_coef_loss = -(log_ent * (log_prob + target_entropy).detach()).mean()
            out["ent_coef_loss"].append(ent_coef_loss.detach())
            opt_e.zero_grad()
            ent_coef_loss.backward()
            out["ent_grads"].append(log_ent.grad.clone())
            opt_e.step()
        else:
            ent_coef = th.tensor(FIXED_ENT_COEF, dtype=th.float64)
            out["ent_coef_loss"].append(th.zeros((), dtype=th.float64))
        out["ent_coef"].append(ent_coef.detach().reshape(()))
        with th.no_grad():
            next_actions, next_log_prob = action_log_prob(nxt, case["eps_next"][g])
            next_q = th.cat([t(th.cat([nxt, next_actions], dim=1)) for t in targets], dim=1)
            next_q, _ = th.min(next_q, dim=1, keepdim=True)
            next_q = next_q - ent_coef * next_log_prob.reshape(-1, 1)
            target_q = rew + (1 - dones) * GAMMA * next_q
        current_q = [c(th.cat([obs, act], dim=1)) for c in critics]
        critic_loss = 0.5 * sum(F.mse_loss(q, target_q) for q in current_q)
        out["critic_loss"].append(critic_loss.detach())
        opt_c.zero_grad()
        critic_loss.backward()
        out["critic_grads"].append(th.cat([p.grad.reshape(-1) for p in critic_params]))
        opt_c.step()
        q_pi = th.cat([c(th.cat([obs, actions_pi], dim=1)) for c in critics], dim=1)
        min_qf_pi, _ = th.min(q_pi, dim=1, keepdim=True)
        actor_loss = (ent_coef * log_prob - min_qf_pi).mean()
        out["actor_loss"].append(actor_loss.detach())
        opt_a.zero_grad()
        actor_loss.backward()
        out["actor_grads"].append(th.cat([p.grad.reshape(-1) for p in actor_params]))
        opt_a.step()
        if g % tui == 0:
            polyak_update(critic_params, target_params, TAU)
    out["params"] = dict(actor=actor_params, critic=critic_params, target=target_params, ent=[log_ent])
    out["opts"] = dict(actor=opt_a, critic=opt_c, ent=opt_e)
    return out


def _check_against_eager(case, tui):
    G = G_MAX
    case = as_double(case)
    e = _eager_steps(case, G, tui)
    close = functools.partial(th.testing.assert_close, rtol=1.3e-6, atol=1e-5)  # torch's fp32 defaults
    L = case["L"]
    st = clone_state(case["state"])
    n = dict(actor=L.n_actor, critic=L.n_critic, ent=1)
    floor = {k: th.zeros(n[k], dtype=th.bool) for k in n}
    one_call = clone_state(case["state"])
    outs3 = run(su.sac_update_reference, case, one_call, G=G, tui=tui, dtype=th.float64)
    for g in range(G):  # step by step, to see every step's gradients
        kept = st["target"].clone()
        outs = run(su.sac_update_reference, case, st, G=1, lo=g, dtype=th.float64)
        if g % tui != 0:  # (a one-step call is step 0 of its launch: undo its Polyak update)
            st["target"].copy_(kept)
        for key in su.OUTPUTS:
            close(outs[key][0], e[key][g])
        for k, eg in (("actor", e["actor_grads"]), ("critic", e["critic_grads"]), ("ent", e["ent_grads"])):
            if st[k] is None:
                continue
            rg = st[k]["grad"][: n[k]]
            close(rg, eg[g])
            both_zero = (eg[g] == 0) & (rg == 0)  # (a dead unit's exact zero has no sign to flip)
            floor[k] |= (eg[g].abs() <= 1e-6 * eg[g].abs().max()) & ~both_zero
    # all three steps in one call are the three single-step calls
    for k in ("actor", "critic", "ent"):
        if st[k] is not None:
            assert th.equal(one_call[k]["flat"], st[k]["flat"]) and th.equal(one_call[k]["grad"], st[k]["grad"])
            assert one_call[k]["flat"].dtype == th.float64
    assert th.equal(one_call["target"], st["target"])
    for key in su.OUTPUTS:
        close(outs3[key], th.stack(e[key]))
    for k in ("actor", "critic", "ent"):
        if st[k] is None:
            continue
        assert float(st[k]["step"]) == G
        opt, ps = e["opts"][k], e["params"][k]
        close(st[k]["m"][: n[k]], th.cat([opt.state[p]["exp_avg"].reshape(-1) for p in ps]))
        close(st[k]["v"][: n[k]], th.cat([opt.state[p]["exp_avg_sq"].reshape(-1) for p in ps]))
        keep = ~floor[k]
        assert int(keep.sum()) > n[k] // 2
        close(st[k]["flat"][: n[k]][keep], th.cat([p.detach().reshape(-1) for p in ps])[keep])
    keep = ~floor["critic"]
    close(st["target"][: n["critic"]][keep],
                            th.cat([p.detach().reshape(-1) for p in e["params"]["target"]])[keep])
    return st, e


@pytest.mark.parametrize("shape", ["p", "h"])
@pytest.mark.parametrize("variant", VARIANTS)
def test_reference_matches_eager_sac_step(shape, variant):
    """Three gradient steps of ``sac_update_reference`` against the eager step with
    ``torch.optim.Adam`` (lr 1e-3) on the same ids and noise, at torch's fp32 ``assert_close``
    defaults: the losses, ``ent_coef``, every step's gradients, the moments, the parameters and the
    target. Both sides run in fp64, so the comparison sees the maths and not fp32 rounding: the
    eager log-prob recovers the noise as ``(u - mean) / std``, which in fp32 is rounding garbage
    where ``log_std`` is clamped at -20 (``std = 2e-9``), and at these magnitudes the fp32 noise of
    a loss alone is of the size of the tolerance. (fp32 is measured on the GPU, against fp64.) An
    element whose gradient sits at Adam's sign-flip floor in some step
    (``|g| <= 1e-6 max|g|``: rounding decides its sign, and with it an update of +-lr) is compared
    through its gradient and moments only, not through its parameter."""
    _check_against_eager(make_case(shape, variant), tui=1)


def test_reference_matches_eager_with_a_target_update_interval():
    """``target_update_interval = 2`` with ``G = 3``: Polyak after steps 0 and 2 only."""
    case = make_case("h", "base", 2)
    st, _ = _check_against_eager(case, tui=2)
    every = clone_state(case["state"], th.float64)
    run(su.sac_update_reference, case, every, G=G_MAX, tui=1, dtype=th.float64)
    assert not th.equal(every["target"], st["target"])


def test_layout_follows_parameter_order():
    from imitation_amd.envs import spaces
    from imitation_amd.rl.sac import SACPolicy

    pol = SACPolicy(spaces.Box(-1, 1, (5,), np.float32), spaces.Box(-1, 1, (2,), np.float32), lambda _: 1e-3,
                    net_arch=dict(pi=[7, 3], qf=[4, 6]))
    L = su.SACLayout.from_params(list(pol.actor.parameters()), list(pol.critic.parameters()))
    assert (L.D, L.A, L.actor_arch, L.critic_arch) == (5, 2, (7, 3), (4, 6))
    assert L.actor_offsets == (0, 35, 42, 63, 66, 72, 74, 80) and L.n_actor == 82
    assert L.critic_offsets == (0, 28, 32, 56, 62, 68, 69, 97, 101, 125, 131, 137) and L.n_critic == 138
    assert L == su.SACLayout.from_dims(5, 2, [7, 3], [4, 6])
    flat = th.cat([p.detach().reshape(-1) for p in pol.actor.parameters()])
    for v, p in zip(L.actor_views(flat), pol.actor.parameters()):
        assert th.equal(v, p.detach())
    assert [n for n, _ in pol.actor.named_parameters()][4:] == ["mu.weight", "mu.bias", "log_std.weight", "log_std.bias"]
    flat = th.cat([p.detach().reshape(-1) for p in pol.critic.parameters()])
    for v, p in zip([v for cv in L.critic_views(flat) for v in cv], pol.critic.parameters()):
        assert th.equal(v, p.detach())
    with pytest.raises(ValueError):
        su.SACLayout.from_params(list(pol.actor.parameters())[:6], list(pol.critic.parameters()))
    with pytest.raises(ValueError):
        su.SACLayout.from_params(list(pol.actor.parameters()), list(pol.critic.parameters())[:6])


# ---- eligibility: every rule keeps the eager step, with its own reason
def _pendulum(n_envs=1):
    from imitation_amd.util.util import make_vec_env

    return make_vec_env("Pendulum-v1", rng=np.random.default_rng(0), n_envs=n_envs)


def _sac(**kwargs):
    from imitation_amd.rl.sac import SAC

    kw = dict(learning_starts=8, batch_size=32, seed=0, device="cpu", policy_kwargs=dict(net_arch=[16, 16]))
    kw.update(kwargs)
    return SAC("MlpPolicy", _pendulum(), **kw)


def _learn_and_path(model):
    p0 = [p.detach().clone() for p in model.actor.parameters()]
    model.learn(12)
    assert model._n_updates > 0
    assert any(not th.equal(a, b.detach()) for a, b in zip(p0, model.actor.parameters())), "the training step did not run"
    return model.update_path


def test_every_eligibility_rule_keeps_the_eager_step(monkeypatch):
    from imitation_amd.envs import spaces
    from imitation_amd.rl import buffers
    from imitation_amd.rl import sac as sac_mod
    from imitation_amd.rl.torch_layers import FlattenExtractor

    class MyFlatten(FlattenExtractor):
        pass

    class MyBuffer(buffers.ReplayBuffer):
        pass

    seen = {}
    arch = dict(net_arch=[16, 16])
    # rules a construction can break
    built = {
        "device": {},
        "net-arch": dict(policy_kwargs=dict(net_arch=[16, 16, 16])),
        "activation": dict(policy_kwargs=dict(activation_fn=nn.Tanh, **arch)),
        "features-extractor": dict(policy_kwargs=dict(features_extractor_class=MyFlatten, **arch)),
        "optimizer": dict(policy_kwargs=dict(optimizer_kwargs=dict(weight_decay=1e-2), **arch)),
        "n-critics": dict(policy_kwargs=dict(n_critics=3, **arch)),
        "replay-buffer": dict(replay_buffer_class=MyBuffer),
        "batch-size": dict(batch_size=257, learning_starts=8),
    }
    for reason, kw in built.items():
        seen[reason] = _learn_and_path(_sac(**kw))
    assert _learn_and_path(_sac(policy_kwargs=dict(net_arch=[65, 64]))) == "eager:net-arch"
    assert _learn_and_path(_sac(policy_kwargs=dict(net_arch=dict(pi=[16, 16], qf=[16])))) == "eager:net-arch"
    assert _learn_and_path(_sac(policy_kwargs=dict(optimizer_kwargs=dict(amsgrad=True), **arch))) == "eager:optimizer"
    assert _learn_and_path(_sac(policy_kwargs=dict(optimizer_class=th.optim.AdamW, **arch))) == "eager:optimizer"
    with monkeypatch.context() as mp:
        mp.setenv("IMITATION_AMD_SAC_FUSED", "0")
        seen["knob"] = _learn_and_path(_sac())
    with monkeypatch.context() as mp:
        mp.setenv("IMITATION_AMD_FUSED", "0")
        seen["kernels-off"] = _learn_and_path(_sac())

    # rules of the run's surroundings: one trained model, the decision taken again under each
    model = _sac()
    assert _learn_and_path(model) == "eager:device"

    def decide_again(reason):
        p0 = [p.detach().clone() for p in model.actor.parameters()]
        model.update_path = None
        model.train(gradient_steps=1, batch_size=32)
        assert any(not th.equal(a, b.detach()) for a, b in zip(p0, model.actor.parameters()))
        seen[reason] = model.update_path

    with monkeypatch.context() as mp:
        mp.setattr(model, "observation_space", spaces.Box(low=0, high=255, shape=(3,), dtype=np.uint8))
        decide_again("obs-space")
    with monkeypatch.context() as mp:
        mp.setattr(model, "action_space", spaces.Box(low=-1, high=1, shape=(62,), dtype=np.float32))  # 3 + 62 > 64
        decide_again("action-space")
    with monkeypatch.context() as mp:
        mp.setattr(model, "use_sde", True)
        decide_again("sde")
    with monkeypatch.context() as mp:
        mp.setattr(sac_mod.pdist, "world_size", lambda: 2)
        mp.setattr(sac_mod.pdist, "allreduce_grads", lambda params: None)
        mp.setattr(model, "_actor_bucket", None)
        decide_again("world-size")
    with monkeypatch.context() as mp:
        mp.setattr(model, "_vec_normalize_env", object())  # (no normalize_obs / normalize_reward: samples pass through)
        decide_again("vec-normalize")

    assert seen == {r: f"eager:{r}" for r in seen}
    assert len(seen) == 15 and len(set(seen.values())) == 15


# ------------------------------------------------------------------------------------ GPU
def _ulp(x: float) -> float:
    return float(np.spacing(np.float32(abs(x))))


def _gpu_state(case, dtype=None):
    return clone_state(case["state"], dtype, device="cuda")


@pytest.mark.gpu
@pytest.mark.parametrize("shape,variant", GRID)
def test_kernel_against_fp64(shape, variant):
    """One step: the four outputs, the critic and actor gradient buckets and the target bucket
    after the Polyak update. Per quantity the kernel's max abs error against the fp64 evaluation
    (``sac_update_reference`` on inputs cast to double) must be within 4 x the error of fp32 torch
    (``sac_update_reference`` in fp32 on the GPU) against the same fp64 values, plus one fp32 ulp of
    the quantity's max magnitude."""
    case = make_case(shape, variant)
    k, e, d = _gpu_state(case), _gpu_state(case), _gpu_state(case, th.float64)
    k_out = run(su.sac_update_step, case, k, device="cuda")
    e_out = run(su.sac_update_reference, case, e, device="cuda")
    d_out = run(su.sac_update_reference, case, d, dtype=th.float64, device="cuda")
    L = case["L"]
    quantities = [(key, k_out[key], e_out[key], d_out[key]) for key in su.OUTPUTS]
    quantities += [("critic grad", k["critic"]["grad"][: L.n_critic], e["critic"]["grad"][: L.n_critic], d["critic"]["grad"][: L.n_critic]),
                   ("actor grad", k["actor"]["grad"][: L.n_actor], e["actor"]["grad"][: L.n_actor], d["actor"]["grad"][: L.n_actor]),
                   ("target", k["target"][: L.n_critic], e["target"][: L.n_critic], d["target"][: L.n_critic])]
    if k["ent"] is not None:
        quantities.append(("ent grad", k["ent"]["grad"][:1], e["ent"]["grad"][:1], d["ent"]["grad"][:1]))
    report = []
    for name, kq, eq, dq in quantities:
        err_k = float((kq.double() - dq).abs().max())
        err_e = float((eq.double() - dq).abs().max())
        bound = 4 * err_e + _ulp(float(dq.abs().max()))
        report.append((name, err_k, err_e, bound))
        print(f"sac_update {shape} {variant} {name}: kernel {err_k:.3e} eager {err_e:.3e} "
              f"ratio {err_k / err_e if err_e else float('inf') if err_k else 0.0:.2f} bound {bound:.3e} "
              f"of-bound {err_k / bound if bound else 0.0:.2f}")
    for name, err_k, err_e, bound in report:
        assert err_k <= bound, (name, err_k, err_e, bound)
    for key in ("actor", "critic"):
        assert not th.isnan(k[key]["flat"]).any()


def _mid_training(state, L):
    n = dict(actor=L.n_actor, critic=L.n_critic, ent=1)
    gen = th.Generator().manual_seed(5)
    for key, step in (("actor", 7.0), ("critic", 9.0), ("ent", 4.0)):
        f = state[key]
        if f is None:
            continue
        f["m"].copy_(th.rand(f["m"].shape, generator=gen) * 0.2 - 0.1)
        f["v"].copy_(th.rand(f["v"].shape, generator=gen) * 0.01)
        f["step"].fill_(step)
        for mom in ("m", "v"):  # (the alignment padding of a FusedAdam bucket is zero)
            f[mom][n[key] :] = 0.0
    return state


@pytest.mark.gpu
@pytest.mark.parametrize("shape,variant", GRID)
def test_adam_handoff_is_adam_flat(shape, variant):
    """Parameters, moments and step counters of the three buckets after the launch are bitwise one
    ``adam_flat`` launch each from the pre-step state and the gradient the kernel left behind; the
    target is the Polyak step of the updated critic."""
    from imitation_amd import ops

    case = make_case(shape, variant)
    pre = _mid_training(clone_state(case["state"]), case["L"])
    pre = clone_state(pre, device="cuda")
    k = clone_state(pre)
    hp = (3e-3, 0.9, 0.999, 1e-8)
    run(su.sac_update_step, case, k, hp=hp, device="cuda")
    ref = clone_state(pre)
    for key, step in (("actor", 8.0), ("critic", 10.0), ("ent", 5.0)):
        if ref[key] is None:
            continue
        f = ref[key]
        f["grad"].copy_(k[key]["grad"])
        cnt = th.zeros(1, dtype=th.int32, device="cuda")
        ops.native().adam_flat(f["flat"], f["grad"], f["m"], f["v"], f["step"], hp[0], hp[1], hp[2], hp[3], 0.0, False, False,
                               False, cnt, None, None, None, None)
        for part in ("flat", "m", "v", "step", "grad"):
            assert th.equal(k[key][part], f[part]), (key, part)
        assert float(k[key]["step"]) == step
        assert float(k[key]["grad"].abs().max()) > 0
    n = case["L"].n_critic
    polyak = pre["target"] * (1 - TAU) + TAU * k["critic"]["flat"]
    th.testing.assert_close(k["target"][:n], polyak[:n])
    assert not th.equal(k["target"], pre["target"])


def _assert_states_equal(s1, s2):
    for key in ("actor", "critic", "ent"):
        if s1[key] is None:
            assert s2[key] is None
            continue
        for part in s1[key]:
            assert th.equal(s1[key][part], s2[key][part]), (key, part)
    assert th.equal(s1["target"], s2["target"])


@pytest.mark.gpu
@pytest.mark.parametrize("shape", list(SHAPES))
@pytest.mark.parametrize("lrs", [(1e-3, 1e-3, 1e-3), (1e-3, 4e-3, 4e-3)])
def test_multi_step_launch_is_single_step_launches(shape, lrs):
    """``G = 3`` in one launch is bitwise three ``G = 1`` launches (``target_update_interval = 1``)
    with the same ids and noise; with the learning rate changed after the first step: a ``G = 1``
    and a ``G = 2`` launch against three."""
    case = make_case(shape, "base")
    hp = lambda lr: (lr, 0.9, 0.999, 1e-8)  # noqa: E731
    one = _gpu_state(case)
    out1 = [run(su.sac_update_step, case, one, G=1, lo=g, hp=hp(lrs[g]), device="cuda") for g in range(3)]
    many = _gpu_state(case)
    if lrs[0] == lrs[1]:
        outs = run(su.sac_update_step, case, many, G=3, hp=hp(lrs[0]), device="cuda")
    else:
        first = run(su.sac_update_step, case, many, G=1, hp=hp(lrs[0]), device="cuda")
        rest = run(su.sac_update_step, case, many, G=2, lo=1, hp=hp(lrs[1]), device="cuda")
        outs = {key: th.cat([first[key], rest[key]]) for key in su.OUTPUTS}
    for key in su.OUTPUTS:
        assert th.equal(outs[key], th.cat([o[key] for o in out1])), key
    _assert_states_equal(one, many)
    assert float(many["actor"]["step"]) == 3.0 and float(many["critic"]["step"]) == 3.0


@pytest.mark.gpu
@pytest.mark.parametrize("shape,variant", GRID)
def test_two_launches_from_equal_states_are_bitwise_equal(shape, variant):
    case = make_case(shape, variant)
    s1, s2 = _gpu_state(case), _gpu_state(case)
    o1 = run(su.sac_update_step, case, s1, G=2, device="cuda")
    o2 = run(su.sac_update_step, case, s2, G=2, device="cuda")
    for key in su.OUTPUTS:
        assert th.equal(o1[key], o2[key]), key
    _assert_states_equal(s1, s2)
    assert not th.equal(s1["actor"]["flat"], case["state"]["actor"]["flat"].cuda())
    assert not th.equal(s1["critic"]["flat"], case["state"]["critic"]["flat"].cuda())


@pytest.mark.gpu
def test_target_bucket_views_follow_polyak_and_load_state_dict():
    """The target critic's parameters are views of the bucket the kernel reads: ``polyak_update``
    and ``load_state_dict`` change the next launch's critic loss (``done = 0``, so the target
    counts), and a rebound parameter is packed again."""
    from imitation_amd.rl.off_policy import polyak_update
    from imitation_amd.rl.sac import SAC

    model = SAC("MlpPolicy", _pendulum(), device="cuda", seed=0, policy_kwargs=dict(net_arch=[64, 64]))
    model._sac_bind()
    L, bucket = model._sac["layout"], model._sac["target"]
    assert (L.D, L.A, L.actor_arch, L.critic_arch) == (3, 1, (64, 64), (64, 64))
    gen = th.Generator().manual_seed(1)
    rows = 32
    src = [t.cuda() for t in (th.randn(rows, 3, generator=gen), th.randn(rows, 3, generator=gen),
                              th.rand(rows, 1, generator=gen) * 2 - 1, th.randn(rows, generator=gen), th.zeros(rows),
                              th.zeros(rows))]
    ids = th.arange(rows, device="cuda").reshape(1, rows)
    eps = [th.randn(1, rows, 1, generator=gen).cuda() for _ in range(2)]

    def buckets():
        opts = (model.actor.optimizer, model.critic.optimizer, model.ent_coef_optimizer)
        return [{k: o._flat[0][k].clone() for k in ("flat", "grad", "m", "v", "step")} for o in opts]

    def loss_now():
        model._sac_bind()
        assert model._sac["target"] is bucket, "in-place updates must not re-pack the bucket"
        packed = th.cat([p.detach().reshape(-1) for p in model.critic_target.parameters()])
        assert th.equal(bucket[: L.n_critic], packed)
        a, c, e = buckets()
        kl = su.sac_update_step(src, None, ids, None, eps[0], eps[1], a, c, e, bucket.clone(), L, gamma=GAMMA)["critic_loss"]
        a, c, e = buckets()
        rl = su.sac_update_reference(src, None, ids, None, eps[0], eps[1], a, c, e, bucket.clone(), L,
                                     gamma=GAMMA)["critic_loss"]
        th.testing.assert_close(kl, rl)
        return float(kl)

    l0 = loss_now()
    sd = {k: v * 1.5 + 0.1 for k, v in model.critic_target.state_dict().items()}
    model.critic_target.load_state_dict(sd)
    l1 = loss_now()
    with th.no_grad():
        for p in model.critic.parameters():
            p.add_(0.2)
    polyak_update(model.critic.parameters(), model.critic_target.parameters(), 0.5)
    l2 = loss_now()
    assert abs(l1 - l0) > 1e-3 and abs(l2 - l1) > 1e-3, (l0, l1, l2)
    # a rebound parameter is packed again
    p = next(model.critic_target.parameters())
    p.data = p.data.clone()
    model._sac_bind()
    assert model._sac["target"] is not bucket and p.data_ptr() == model._sac["target"].data_ptr()


@pytest.mark.gpu
@pytest.mark.parametrize("what", ["B=257", "DA=65", "H1=65", "H2=65"])
def test_launcher_limits_raise_and_launch_nothing(what):
    dims = dict(D=4, A=2, H1=8, H2=8, B=4)
    key, val = what.split("=")
    if key == "DA":
        dims["D"] = int(val) - dims["A"]
    else:
        dims[key] = int(val)
    L = su.SACLayout.from_dims(dims["D"], dims["A"], (dims["H1"], dims["H2"]))
    rows = 8
    src = [th.zeros(rows, dims["D"]), th.zeros(rows, dims["D"]), th.zeros(rows, dims["A"]), th.zeros(rows), th.zeros(rows),
           th.zeros(rows)]
    src = [t.cuda() for t in src]
    st = dict(actor=_bucket(L.n_actor), critic=_bucket(L.n_critic), ent=_bucket(1), target=th.zeros(L.n_critic + (-L.n_critic) % 4))
    st = clone_state(st, device="cuda")
    for key in ("actor", "critic", "ent"):
        for part in ("flat", "grad", "m", "v"):
            st[key][part].fill_(0.5)
    st["target"].fill_(0.5)
    before = clone_state(st)
    ids = th.zeros((1, dims["B"]), dtype=th.int64, device="cuda")
    eps = th.zeros((1, dims["B"], dims["A"]), device="cuda")
    with pytest.raises(RuntimeError, match="sac_update_step"):
        su.sac_update_step(src, None, ids, None, eps, eps.clone(), st["actor"], st["critic"], st["ent"], st["target"], L)
    th.cuda.synchronize()
    _assert_states_equal(st, before)
