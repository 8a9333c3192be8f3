"""The fused BC minibatch steps (``imitation_amd.ops.bc_mlp``; ``csrc/kernels/bc_mlp.hip``).

CPU part: ``bc_mlp_reference`` is the maths of the eager BC step (``BehaviorCloningLossCalculator``
on a real policy, ``backward``, ``torch.optim.Adam``), the layout follows parameter identity and
every limit raises. GPU part: the kernel against an fp64 evaluation, its Adam hand-off,
multi-step launches, determinism, the untouched gradient bucket and the launcher's limits."""

import copy
import functools

import numpy as np
import pytest
import torch as th
from torch import nn

from imitation_amd.algorithms.bc import BehaviorCloningLossCalculator
from imitation_amd.envs import spaces
from imitation_amd.ops import bc_mlp
from imitation_amd.ops.optim import FusedAdam
from imitation_amd.ops.rl import BC_METRICS
from imitation_amd.rl.policies import ActorCriticPolicy

# name -> (D, pi, vf, activation, B, {head: A}); every bucket holds the value net (and log_std)
SHAPES = {
    "a": (4, [32, 32], [32, 32], nn.Tanh, 32, {"cat": 2}),        # CartPole default
    "b": (17, [32, 32], [32, 32], nn.Tanh, 32, {"gauss": 6}),     # HalfCheetah
    "c": (3, [5, 7], [3], nn.ReLU, 1, {"cat": 3, "gauss": 1}),    # unpadded bucket length % 4 != 0
    "d": (61, [64, 64], [64, 64], nn.Tanh, 130, {"cat": 18, "gauss": 18}),  # two full chunks + 2 rows
    "e": (64, [64, 64], [64, 64], nn.ReLU, 256, {"cat": 64, "gauss": 64}),  # the limits
}
CASES = [(s, h) for s, v in SHAPES.items() for h in v[5]]
WEIGHTS = [(1e-3, 0.0), (1e-3, 3e-5), (0.0, 3e-5)]  # (ent_weight, l2_weight)
KEYS = ("flat", "grad", "m", "v", "step")


def make_policy(shape, head, seed=0):
    D, pi, vf, act, _, heads = SHAPES[shape]
    A = heads[head]
    th.manual_seed(seed)
    obs_space = spaces.Box(low=-np.inf, high=np.inf, shape=(D,), dtype=np.float32)
    act_space = spaces.Discrete(A) if head == "cat" else spaces.Box(low=-1.0, high=1.0, shape=(A,), dtype=np.float32)
    policy = ActorCriticPolicy(obs_space, act_space, lambda _: 1e-3, net_arch=dict(pi=pi, vf=vf), activation_fn=act)
    gen = th.Generator().manual_seed(seed + 1)
    with th.no_grad():  # every term matters: a head at scale ~0.5 (not the 0.01 init), log_std in [-1, 0.5]
        policy.action_net.weight.copy_(th.rand(policy.action_net.weight.shape, generator=gen) - 0.5)
        policy.action_net.bias.copy_(th.rand(A, generator=gen) - 0.5)
        if head == "gauss":
            policy.log_std.copy_(th.rand(A, generator=gen) * 1.5 - 1.0)
    return policy


@functools.lru_cache(maxsize=None)
def _base_case(shape, head, G, seed):
    D, _, _, _, B, heads = SHAPES[shape]
    A = heads[head]
    policy = make_policy(shape, head, seed)
    eager = copy.deepcopy(policy)  # (its own storage: FusedAdam re-points the original's parameters)
    opt = FusedAdam(policy.parameters(), lr=1e-3)
    L = bc_mlp.BCMlpLayout.from_policy(policy, opt)
    f = opt._flat[0]
    gen = th.Generator().manual_seed(seed + 2)
    rows = max(B + 8, 40)
    obs = th.randn(rows, D, generator=gen)
    if head == "cat":
        acts = th.randint(0, A, (rows,), generator=gen)
    else:  # within a few sigma of the mean
        with th.no_grad():
            mean = policy.get_distribution(obs).mean_actions
            acts = mean + th.exp(policy.log_std) * th.randn(rows, A, generator=gen) * 1.5
    ids = th.randint(0, rows, (G, B), generator=gen)
    if B > 1:
        ids[:, 1] = ids[:, 0]  # a duplicate row in every batch
    state = dict(flat=f["flat"].clone(), grad=th.zeros_like(f["flat"]), m=th.zeros_like(f["flat"]),
                 v=th.zeros_like(f["flat"]), step=th.zeros(1))
    views = [(off, k) for off, k, _ in f["views"]]
    return dict(L=L, obs=obs, acts=acts, ids=ids, state=state, eager=eager, views=views, n=f["n"])


def make_case(shape, head, G=1, seed=0, device="cpu"):
    c = _base_case(shape, head, G, seed)  # (built once and left unchanged: everything below is a copy)
    return dict(c, obs=c["obs"].to(device), acts=c["acts"].to(device), ids=c["ids"].to(device),
                state={k: v.to(device) for k, v in c["state"].items()})


def clone_state(state, dtype=None):
    return {k: (v.clone() if dtype is None else v.to(dtype)) for k, v in state.items()}


def mid_training(state, n):
    """A state in mid-training: nonzero moments, step 7 (the alignment padding stays zero)."""
    gen = th.Generator().manual_seed(5)
    st = clone_state(state)
    st["m"].copy_((th.rand(st["m"].shape, generator=gen) * 0.2 - 0.1).to(st["m"].device))
    st["v"].copy_((th.rand(st["v"].shape, generator=gen) * 0.01).to(st["v"].device))
    st["m"][n:] = 0.0
    st["v"][n:] = 0.0
    st["step"].fill_(7.0)
    return st


def run(fn, case, state, weights, lr=1e-3, ids=None, keep_grad=False):
    return fn(case["obs"], case["acts"], case["ids"] if ids is None else ids, state["flat"], state["grad"], state["m"],
              state["v"], state["step"], case["L"], lr=lr, ent_weight=weights[0], l2_weight=weights[1], keep_grad=keep_grad)


# ------------------------------------------------------------------------------------ CPU
@pytest.mark.parametrize("shape,head", [c for c in CASES if c[0] in "abc"])
@pytest.mark.parametrize("weights", WEIGHTS)
def test_reference_matches_eager_bc_step(shape, head, weights):
    """One step of ``bc_mlp_reference`` against the real eager step on the same rows
    (``BehaviorCloningLossCalculator`` on a real policy, ``backward``, ``th.optim.Adam``), at
    torch's fp32 ``assert_close`` defaults: all seven metrics, every gradient (the value net's L2
    gradient and ``log_std``'s included), the moments and the parameters. An element whose
    gradient sits at Adam's sign-flip floor (``|g| <= 1e-6 max|g|``) is compared through its
    gradient and moments only."""
    lr = 1e-3
    case = make_case(shape, head)
    policy = copy.deepcopy(case["eager"])
    opt = th.optim.Adam(policy.parameters(), lr=lr)
    rows = case["ids"][0]
    m = BehaviorCloningLossCalculator(*weights)(policy, case["obs"][rows], case["acts"][rows])
    m.loss.backward()
    st = clone_state(case["state"])
    out = run(bc_mlp.bc_mlp_reference, case, st, weights, lr=lr, keep_grad=True)
    for i, k in enumerate(BC_METRICS):
        th.testing.assert_close(out[0, i], getattr(m, k).detach().reshape(()), msg=lambda s, k=k: f"{k}: {s}")
    n = case["n"]
    e_grad = th.zeros(n)
    for p, (off, k) in zip(policy.parameters(), case["views"]):
        if p.grad is not None:
            e_grad[off : off + k] = p.grad.reshape(-1)
    th.testing.assert_close(st["grad"][:n], e_grad)
    if weights[1] != 0.0:
        assert float(policy.value_net.weight.grad.abs().min()) > 0  # (the pure L2 gradient of the unused value net)
    if head == "gauss":
        assert float(policy.log_std.grad.abs().min()) > 0
    opt.step()
    e_p = th.cat([p.detach().reshape(-1) for p in policy.parameters()])
    e_m = th.cat([opt.state[p]["exp_avg"].reshape(-1) if p in opt.state else th.zeros(p.numel()) for p in policy.parameters()])
    e_v = th.cat([opt.state[p]["exp_avg_sq"].reshape(-1) if p in opt.state else th.zeros(p.numel()) for p in policy.parameters()])
    th.testing.assert_close(st["m"][:n], e_m)
    th.testing.assert_close(st["v"][:n], e_v)
    ok = (e_grad.abs() > 1e-6 * e_grad.abs().max()) | ((e_grad == 0) & (st["grad"][:n] == 0))
    assert int(ok.sum()) > n // 2
    th.testing.assert_close(st["flat"][:n][ok], e_p[ok])
    assert float(st["step"]) == 1.0
    # without keep_grad the gradient bucket is not touched
    st2 = clone_state(case["state"])
    st2["grad"].fill_(0.5)
    out2 = run(bc_mlp.bc_mlp_steps, case, st2, weights, lr=lr)
    assert th.equal(out2, out) and th.equal(st2["flat"], st["flat"]) and bool((st2["grad"] == 0.5).all())


def test_reference_multi_step_is_single_steps():
    case = make_case("b", "gauss", G=3)
    one, many = clone_state(case["state"]), clone_state(case["state"])
    rows = [run(bc_mlp.bc_mlp_reference, case, one, WEIGHTS[1], ids=case["ids"][g : g + 1]) for g in range(3)]
    out = run(bc_mlp.bc_mlp_reference, case, many, WEIGHTS[1])
    assert th.equal(out, th.cat(rows))
    for k in KEYS:
        assert th.equal(one[k], many[k]), k
    assert float(many["step"]) == 3.0


def test_layout_follows_parameter_identity():
    policy = make_policy("c", "gauss")
    params = list(policy.parameters())
    order = params[::-1]  # not policy.parameters() order
    opt = FusedAdam(order, lr=1e-3)
    L = bc_mlp.BCMlpLayout.from_policy(policy, opt)
    flat = opt._flat[0]["flat"]
    assert (L.D, L.H1, L.H2, L.A, L.gaussian, L.tanh) == (3, 5, 7, 1, True, False)
    assert L.n == flat.numel() and opt._flat[0]["n"] % 4 != 0
    pn = policy.mlp_extractor.policy_net
    want = [pn[0].weight, pn[0].bias, pn[2].weight, pn[2].bias, policy.action_net.weight, policy.action_net.bias]
    for v, p in zip(L.views(flat), want):
        assert v.data_ptr() == p.data_ptr() and th.equal(v, p.detach())
    assert L.log_std_view(flat).data_ptr() == policy.log_std.data_ptr()
    straight = make_policy("c", "gauss")
    L2 = bc_mlp.BCMlpLayout.from_policy(straight, FusedAdam(straight.parameters(), lr=1e-3))
    assert L2.offsets != L.offsets
    # a policy parameter that is not in the bucket
    partial = make_policy("c", "cat")
    with pytest.raises(ValueError, match="not in the optimizer's flat bucket"):
        bc_mlp.BCMlpLayout.from_policy(partial, FusedAdam(list(partial.parameters())[2:], lr=1e-3))


def _policy_with(pi, D=4, A=2, act=nn.Tanh, vf=(8,)):
    obs_space = spaces.Box(low=-np.inf, high=np.inf, shape=(D,), dtype=np.float32)
    return ActorCriticPolicy(obs_space, spaces.Discrete(A), lambda _: 1e-3, net_arch=dict(pi=list(pi), vf=list(vf)),
                             activation_fn=act)


@pytest.mark.parametrize("what,kw", [
    ("D=65", dict(pi=[8, 8], D=65)), ("H1=65", dict(pi=[65, 8])), ("H2=65", dict(pi=[8, 65])), ("A=65", dict(pi=[8, 8], A=65)),
    ("bucket", dict(pi=[8, 8], vf=[256, 256])), ("trunk", dict(pi=[8, 8, 8])), ("trunk", dict(pi=[8])),
    ("trunk", dict(pi=[8, 8], act=nn.ELU)),
])
def test_every_layout_limit_raises(what, kw):
    policy = _policy_with(**kw)
    with pytest.raises(ValueError, match=what):
        bc_mlp.BCMlpLayout.from_policy(policy, FusedAdam(policy.parameters(), lr=1e-3))


@pytest.mark.parametrize("what", ["B=257", "B=0", "G=0", "n"])
def test_every_call_limit_raises_on_the_cpu(what):
    case = make_case("a", "cat")
    st = clone_state(case["state"])
    before = clone_state(st)
    ids = {"B=257": th.zeros(1, 257, dtype=th.int64), "B=0": th.zeros(1, 0, dtype=th.int64),
           "G=0": th.zeros(0, 32, dtype=th.int64), "n": case["ids"]}[what]
    if what == "n":
        st = {k: (th.cat([v, v.new_zeros(4)]) if k != "step" else v) for k, v in st.items()}
        before = clone_state(st)
    with pytest.raises(ValueError):
        run(bc_mlp.bc_mlp_steps, case, st, WEIGHTS[0], ids=ids)
    for k in KEYS:
        assert th.equal(st[k], before[k]), k


# ------------------------------------------------------------------------------------ GPU
GRID = [(s, h, w) for s, h in CASES for w in WEIGHTS]


def _ulp(x: float) -> float:
    return float(np.spacing(np.float32(abs(x))))


@pytest.mark.gpu
@pytest.mark.parametrize("shape,head,weights", GRID)
def test_kernel_against_fp64(shape, head, weights):
    """The seven metrics and the gradient bucket (``keep_grad``) after one step. Per quantity the
    kernel's max abs error against the fp64 evaluation (``bc_mlp_reference`` on a state cast to
    double) must be within 4 x the error of fp32 torch eager (``bc_mlp_reference`` in fp32 on the
    GPU) against the same fp64 values, plus one fp32 ulp of the quantity's max magnitude."""
    case = make_case(shape, head, device="cuda")
    k, e, d = clone_state(case["state"]), clone_state(case["state"]), clone_state(case["state"], th.float64)
    k_out = run(bc_mlp.bc_mlp_steps, case, k, weights, keep_grad=True)
    e_out = run(bc_mlp.bc_mlp_reference, case, e, weights, keep_grad=True)
    d_out = run(bc_mlp.bc_mlp_reference, case, d, weights, keep_grad=True)
    n = case["n"]
    quantities = [(name, k_out[0, i], e_out[0, i], d_out[0, i]) for i, name in enumerate(BC_METRICS)]
    quantities.append(("grad", k["grad"][:n], e["grad"][:n], d["grad"][:n]))
    report = []
    for name, kq, eq, dq in quantities:
        err_k = float((kq.double() - dq).abs().max())
        err_e = float((eq.double() - dq).abs().max())
        bound = 4 * err_e + _ulp(float(dq.abs().max()))
        report.append((name, err_k, err_e, bound))
        print(f"bc_mlp {shape} {head} ent={weights[0]} l2={weights[1]} {name}: kernel {err_k:.3e} eager {err_e:.3e} "
              f"ratio {err_k / err_e if err_e else float('inf'):.2f} bound {bound:.3e}")
    for name, err_k, err_e, bound in report:
        assert err_k <= bound, (name, err_k, err_e, bound)
    assert not th.isnan(k["flat"]).any() and float(k["step"]) == 1.0
    assert float(d["grad"][:n].abs().max()) > 0


@pytest.mark.gpu
@pytest.mark.parametrize("shape,head,weights", GRID)
def test_adam_handoff_is_adam_flat(shape, head, weights):
    """From a mid-training state, parameters, moments, step counter and gradient bucket after a
    ``keep_grad`` launch are bitwise one ``adam_flat`` launch from the pre-step state and the
    gradient the kernel wrote."""
    from imitation_amd import ops

    case = make_case(shape, head, device="cuda")
    pre = mid_training(case["state"], case["n"])
    k = clone_state(pre)
    run(bc_mlp.bc_mlp_steps, case, k, weights, lr=3e-3, keep_grad=True)
    ref = clone_state(pre)
    ref["grad"].copy_(k["grad"])
    cnt = th.zeros(1, dtype=th.int32, device="cuda")
    ops.native().adam_flat(ref["flat"], ref["grad"], ref["m"], ref["v"], ref["step"], 3e-3, 0.9, 0.999, 1e-8, 0.0, False,
                           False, False, cnt, None, None, None, None)
    for key in KEYS:
        assert th.equal(k[key], ref[key]), key
    assert float(k["step"]) == 8.0 and not th.equal(k["flat"], pre["flat"])


@pytest.mark.gpu
@pytest.mark.parametrize("shape,head", CASES)
@pytest.mark.parametrize("lrs", [(1e-3, 1e-3, 1e-3), (1e-3, 4e-3, 4e-3)])
def test_multi_step_launch_is_single_step_launches(shape, head, lrs):
    """``G = 3`` in one launch is bitwise three ``G = 1`` launches with the same row ids, metrics
    rows included; with the learning rate changed after the first step: a ``G = 1`` and a
    ``G = 2`` launch against the three. (What makes the engine's run-length cap a scheduling choice.)"""
    w = WEIGHTS[1]
    case = make_case(shape, head, G=3, device="cuda")
    ids = lambda lo, hi: case["ids"][lo:hi].contiguous()  # noqa: E731
    pre = mid_training(case["state"], case["n"])
    one = clone_state(pre)
    rows = [run(bc_mlp.bc_mlp_steps, case, one, w, lr=lrs[g], ids=ids(g, g + 1)) for g in range(3)]
    many = clone_state(pre)
    if lrs[0] == lrs[1]:
        out = run(bc_mlp.bc_mlp_steps, case, many, w, lr=lrs[0])
    else:
        out = th.cat([run(bc_mlp.bc_mlp_steps, case, many, w, lr=lrs[0], ids=ids(0, 1)),
                      run(bc_mlp.bc_mlp_steps, case, many, w, lr=lrs[1], ids=ids(1, 3))])
    assert th.equal(out, th.cat(rows)) and bool(th.isfinite(out).all())
    for key in KEYS:
        assert th.equal(one[key], many[key]), key
    assert float(many["step"]) == 10.0
    assert not th.equal(out[0], out[2])


@pytest.mark.gpu
@pytest.mark.parametrize("shape,head", CASES)
def test_two_launches_from_equal_states_are_bitwise_equal_and_leave_the_gradient_bucket(shape, head):
    case = make_case(shape, head, G=2, device="cuda")
    s1, s2 = clone_state(case["state"]), clone_state(case["state"])
    s1["grad"].fill_(0.25)  # without keep_grad the gradient bucket is neither read nor written
    s2["grad"].fill_(-3.0)
    o1 = run(bc_mlp.bc_mlp_steps, case, s1, WEIGHTS[1])
    o2 = run(bc_mlp.bc_mlp_steps, case, s2, WEIGHTS[1])
    assert th.equal(o1, o2)
    for key in ("flat", "m", "v", "step"):
        assert th.equal(s1[key], s2[key]), key
    assert bool((s1["grad"] == 0.25).all()) and bool((s2["grad"] == -3.0).all())
    assert not th.equal(s1["flat"], case["state"]["flat"])


@pytest.mark.gpu
@pytest.mark.parametrize("what", ["B=257", "D=65", "H1=65", "H2=65", "A=65", "n=65540", "G=0"])
def test_launcher_limits_raise_and_launch_nothing(what):
    dims = dict(D=4, H1=8, H2=8, A=2, B=4, n=0, G=1)
    key, val = what.split("=")
    dims[key] = int(val)
    D, H1, H2, A = dims["D"], dims["H1"], dims["H2"], dims["A"]
    sizes = [H1 * D, H1, H2 * H1, H2, A * H2, A]
    offs = tuple(int(x) for x in np.cumsum([0] + sizes[:-1]))
    n = dims["n"] or (sum(sizes) + (-sum(sizes)) % 4)
    L = bc_mlp.BCMlpLayout(D, H1, H2, A, False, True, offs, -1, n)
    rows = 8
    obs = th.zeros(rows, D, device="cuda")
    acts = th.zeros(rows, dtype=th.int64, device="cuda")
    st = {k: th.full((n,), 0.5, device="cuda") for k in ("flat", "grad", "m", "v")}
    st["step"] = th.zeros(1, device="cuda")
    before = clone_state(st)
    ids = th.zeros((dims["G"], dims["B"]), dtype=th.int64, device="cuda")
    with pytest.raises(RuntimeError, match="bc_mlp_steps"):
        bc_mlp.bc_mlp_steps(obs, acts, ids, st["flat"], st["grad"], st["m"], st["v"], st["step"], L, lr=1e-3, keep_grad=True)
    th.cuda.synchronize()
    for k in st:
        assert th.equal(st[k], before[k]), k
