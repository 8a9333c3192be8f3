"""The fused GAIL discriminator plan (``DiscPlan``: csrc/kernels/disc.hip, the discriminator
instance of csrc/kernels/tmlp.hip, csrc/bind/disc.cpp) against
``imitation_amd.testing.disc_reference``.

CPU part: the float64 reference against the eager host path (``RunningNorm.update_stats``,
autograd BCE through ``nn.Sequential``, ``torch.optim.Adam``, ``compute_train_stats``), and
``disc_plan_sizes`` against the documented launch geometry. GPU part: plans built from plain
tensors (no trainer, environment or rollout), every launch of the plan checked on its own and
the fused ``update`` against the staged sequence."""

import functools
import math
from types import SimpleNamespace

import pytest
import torch as th
from torch import nn

from imitation_amd.testing import disc_reference as dref

gpu = pytest.mark.gpu
F64 = th.float64
N_EXPERT, N_GEN = 300, 200
ACT_CODE = {"relu": 1, "tanh": 2}
LR, BETA1, BETA2, ADAM_EPS, REW_EPS = 1e-3, 0.9, 0.999, 1e-8, 1e-5
ADAM_STEPS_TAKEN = 2  # the update under test is optimizer step 3
# Placement of the hidden ReLU pre-activations and of the logits relative to 0 (make_case)
RELU_GAP, LOGIT_STD, LOGIT_MEAN = 4.5, 0.4, 1.2
# cases whose rounding error leaves room for predictions of both kinds (test_reference_conditions)
LOGIT_MEAN_OF = {"state_only_1layer": 0.6, "action_only": 0.5, "baseline": 0.9, "widest_input": 0.9}
# Two rows need less of a gap to keep all their units clear of 0, and have no other rows to
# average the rounding of the active units' offset away in the loss.
RELU_GAP_OF = {"tiny": 2.5}

# name -> obs_dim, action (width, discrete), layout "s a n d", hidden dims, activation, batch,
# minibatch, waves of the fwd/bwd instance
CASES = {
    "baseline": (17, (6, False), "sa", [32, 32], "relu", 256, 256, 4),
    "ragged": (11, (3, False), "sand", [32, 32], "relu", 40, 40, 4),
    "three_mb": (17, (6, False), "sa", [32, 32], "relu", 288, 96, 4),
    "discrete": (4, (3, True), "sand", [64, 64], "tanh", 80, 40, 4),
    "action_only": (5, (2, False), "a", [32], "relu", 64, 64, 4),
    "state_only_1layer": (9, (1, False), "s", [], "relu", 33, 33, 4),
    "two_wave": (17, (6, False), "sa", [128, 100, 128], "tanh", 80, 40, 2),
    # Two layers whose widest dimension pads to 128 (the input here, the hidden layer below):
    # a 4-wave LDS image of exactly 160 KiB. With the 128 bytes of static statistics scratch
    # of the discriminator instance that is over a CU's LDS, so these take the 2-wave instance.
    "widest_input": (60, (8, False), "san", [32], "relu", 64, 64, 2),
    "lds_boundary": (17, (6, False), "sa", [128], "relu", 64, 64, 2),
    "tiny": (3, (1, False), "sa", [32, 32], "relu", 2, 1, 4),
}
CASE_NAMES = list(CASES)
CASE_SEEDS = {n: i for i, n in enumerate(CASE_NAMES)}


def _layout(name):
    D, (A, discrete), lay, hidden, act, B, mb, waves = CASES[name]
    L = dict(obs_dim=D, act_width=A, use_state=int("s" in lay), use_action=int("a" in lay),
             use_next_state=int("n" in lay), use_done=int("d" in lay), act_discrete=int(discrete))
    din = D * L["use_state"] + A * L["use_action"] + D * L["use_next_state"] + L["use_done"]
    return L, [din] + hidden + [1]


def _source(gen, rows, D, A, discrete):
    def obs():
        o = th.randn(rows, D, generator=gen)
        o[:, 0] = 100.0 + o[:, 0]         # far off-centre
        o[:, 1] = 3.0 + 0.05 * o[:, 1]    # off-centre, small spread
        o[:, 2] = 1.5                     # constant: variance exactly 0
        return o

    acts = th.randint(0, A, (rows,), generator=gen) if discrete else th.randn(rows, A, generator=gen).clamp(-1, 1)
    return dict(obs=obs(), acts=acts, next_obs=obs(), dones=th.rand(rows, generator=gen) < 0.3)


def _warm_norm(gen, centre, spread):
    """A norm that has seen 5000 rows of roughly this data."""
    k = centre.numel()
    return dict(mean=(centre + 0.3 * spread * th.randn(k, generator=gen)).float(),
                var=(spread**2 * (0.5 + th.rand(k, generator=gen))).float(), count=5000)


def _fresh_norm(k):
    return dict(mean=th.zeros(k), var=th.ones(k), count=0)


@functools.lru_cache(maxsize=None)
def make_case(name, warm=False, weight_decay=0.0):
    """CPU tensors of one configuration (float32 / int64 / bool, as the plan takes them)."""
    D, (A, discrete), lay, hidden, act, B, mb, waves = CASES[name]
    L, dims = _layout(name)
    gen = th.Generator().manual_seed(CASE_SEEDS[name])
    expert = _source(gen, N_EXPERT, D, A, discrete)
    gens = _source(gen, N_GEN, D, A, discrete)
    e_idx = th.randint(0, N_EXPERT, (B,), generator=gen)
    g_idx = th.randint(0, N_GEN, (B,), generator=gen)
    e_idx[0], e_idx[-1], g_idx[0], g_idx[-1] = 0, N_EXPERT - 1, N_GEN - 1, 0  # first / last row of each set
    if B >= 4:
        e_idx[2], g_idx[2] = e_idx[1], g_idx[1]  # repeats
    Ws, bs = [], []
    for i, o in zip(dims[:-1], dims[1:]):  # nn.Linear's default range
        Ws.append(((th.rand(o, i, generator=gen) * 2 - 1) / math.sqrt(i)).bfloat16().float())
        bs.append((th.rand(o, generator=gen) * 2 - 1) / math.sqrt(i))
    n_params = sum(w.numel() + b.numel() for w, b in zip(Ws, bs))
    # column centres / spreads of the gathered input, for the warm norms
    x_all = th.cat([dref.gather_rows(expert, th.arange(N_EXPERT), L), dref.gather_rows(gens, th.arange(N_GEN), L)])
    centre, spread = x_all.mean(0), x_all.std(0).clamp_min(0.05)
    # Biases that keep every comparison with 0 clear of the bf16 rounding error. A ReLU unit
    # whose pre-activation changes sign under rounding moves its gradients by a whole row's
    # contribution, and a logit that does moves a count: neither says anything about the
    # kernel, and the bounds below are against float64. So every hidden ReLU unit sits
    # RELU_GAP spreads of its pre-activation to one side of 0 (about half on, half off), and
    # the logits have spread LOGIT_STD around LOGIT_MEAN. test_reference_conditions asserts on
    # the two reference modes that no unit flips and how few logits can. The hidden weights
    # are bf16 values, which keeps the common offset of the active units from dominating the
    # rounding error.
    h = ((x_all - centre) / spread).float()
    for l, (W, b) in enumerate(zip(Ws, bs)):
        z = h @ W.T
        if l == len(Ws) - 1:
            W *= LOGIT_STD / z.std(0)
            z = h @ W.T
            b.copy_(-z.mean(0) + LOGIT_MEAN_OF.get(name, LOGIT_MEAN))
        elif act == "relu":
            sign = (th.rand(b.shape, generator=gen) < 0.5).float() * 2 - 1
            b.copy_(-z.mean(0) + sign * RELU_GAP_OF.get(name, RELU_GAP) * z.std(0).clamp_min(1e-3))
        h = z + b
        h = h.clamp_min(0) if act == "relu" else th.tanh(h)
    if warm:
        rew = _warm_norm(gen, centre, spread)
        pol = _warm_norm(gen, centre[:D], spread[:D]) if L["use_state"] else _fresh_norm(D)
    else:
        rew, pol = _fresh_norm(dims[0]), _fresh_norm(D)
    adam = dict(exp_avg=1e-3 * th.randn(n_params, generator=gen), exp_avg_sq=1e-6 * th.rand(n_params, generator=gen),
                step=ADAM_STEPS_TAKEN, lr=LR, beta1=BETA1, beta2=BETA2, eps=ADAM_EPS, weight_decay=weight_decay)
    return SimpleNamespace(name=name, layout=L, dims=dims, act=act, B=B, mb=mb, n_mb=B // mb, waves=waves,
                           expert=expert, gen=gens, e_idx=e_idx, g_idx=g_idx, Ws=Ws, bs=bs, n_params=n_params,
                           rew=rew, pol=pol, adam=adam)


@functools.lru_cache(maxsize=None)
def reference(name, warm=False, weight_decay=0.0, bf16=False, merge_rew=True, merge_pol=True, no_rew=False):
    c = make_case(name, warm, weight_decay)
    return dref.disc_update_reference(
        expert=c.expert, gen=c.gen, e_idx=c.e_idx, g_idx=c.g_idx, layout=c.layout, batch=c.B, minibatch=c.mb,
        Ws=c.Ws, bs=c.bs, hidden_act=c.act, rew_norm=None if no_rew else c.rew, pol_norm=c.pol, rew_eps=REW_EPS,
        adam=c.adam, merge_rew=merge_rew, merge_pol=merge_pol, bf16_operands=bf16)


def logit_tau(name, warm, **kw):
    """(tau, rows of the last minibatch whose reference logit is within tau of 0): tau is 4x the
    largest difference between the float64 and the bf16-operand logits."""
    z, zb = reference(name, warm, **kw)["logits"][-1], reference(name, warm, bf16=True, **kw)["logits"][-1]
    tau = 4.0 * float((z - zb).abs().max())
    return tau, int((z.abs() < tau).sum())


def grad_errors(g, name, warm, **kw):
    """max-abs and L2 error of ``g`` and of the bf16-operand mode against the float64 gradient."""
    ref, bf = reference(name, warm, **kw)["grads"], reference(name, warm, bf16=True, **kw)["grads"]
    e, eb = g.double().cpu() - ref, bf - ref
    return (float(e.abs().max()), float(e.norm())), (float(eb.abs().max()), float(eb.norm()))


def assert_grads(g, name, warm, **kw):
    ref = reference(name, warm, **kw)["grads"]
    g = g.double().cpu()
    (emax, el2), (bmax, bl2) = grad_errors(g, name, warm, **kw)
    print(f"{name} warm={warm} {kw}: kernel err max {emax:.3e} l2 {el2:.3e}; bf16 mode max {bmax:.3e} l2 {bl2:.3e}; "
          f"ratios {emax / bmax:.2f} {el2 / bl2:.2f}")
    th.testing.assert_close(g, ref, rtol=2e-2, atol=2.5e-3 * float(ref.abs().max()))
    assert float(th.nn.functional.cosine_similarity(g, ref, dim=0)) > 0.9999
    # no worse than 4x what rounding the MFMA operands to bf16 costs by itself
    assert emax <= 4.0 * bmax and el2 <= 4.0 * bl2, (emax / bmax, el2 / bl2)


def stats_to_logged(v, c):
    """(loss, entropy) as ``train_disc`` logs them, from the six sums of the last minibatch."""
    rows = 2 * c.mb
    return float(v[0]) / rows * (c.mb / c.B), float(v[5]) / rows


# ------------------------------------------------------------------ CPU: the reference itself

WARM = [False, True]
EAGER_CASES = ["baseline", "three_mb", "discrete", "ragged", "state_only_1layer", "action_only"]


def _eager_host_update(c):
    """``AdversarialTrainer.train_disc`` with the library's own host pieces, in float32 on the CPU."""
    import torch.nn.functional as F

    from imitation_amd.algorithms.adversarial.common import compute_train_stats
    from imitation_amd.util.networks import RunningNorm

    L = c.layout

    def norm_of(state, k):
        m = RunningNorm(k, eps=REW_EPS)
        m.running_mean.copy_(state["mean"])
        m.running_var.copy_(state["var"])
        m.count.fill_(state["count"])
        return m.train()

    rn, pn = norm_of(c.rew, c.dims[0]), norm_of(c.pol, L["obs_dim"])
    layers = []
    for l, (W, b) in enumerate(zip(c.Ws, c.bs)):
        lin = nn.Linear(W.shape[1], W.shape[0])
        with th.no_grad():
            lin.weight.copy_(W)
            lin.bias.copy_(b)
        layers.append(lin)
        if l < len(c.Ws) - 1:
            layers.append(nn.ReLU() if c.act == "relu" else nn.Tanh())
    mlp = nn.Sequential(*layers)
    params = [p for lin in mlp if isinstance(lin, nn.Linear) for p in (lin.weight, lin.bias)]
    a = c.adam
    opt = th.optim.Adam(params, lr=a["lr"], betas=(a["beta1"], a["beta2"]), eps=a["eps"], weight_decay=a["weight_decay"])
    off = 0
    for p in params:
        k = p.numel()
        opt.state[p] = dict(step=th.tensor(float(a["step"])), exp_avg=a["exp_avg"][off:off + k].view_as(p).clone(),
                            exp_avg_sq=a["exp_avg_sq"][off:off + k].view_as(p).clone())
        off += k

    def rows(src, idx):
        cols = []
        if L["use_state"]:
            cols.append(src["obs"][idx])
        if L["use_action"]:
            cols.append(F.one_hot(src["acts"][idx], L["act_width"]).float() if L["act_discrete"] else src["acts"][idx])
        if L["use_next_state"]:
            cols.append(src["next_obs"][idx])
        if L["use_done"]:
            cols.append(src["dones"][idx].float()[:, None])
        return th.cat(cols, 1)

    labels = th.cat([th.ones(c.mb), th.zeros(c.mb)])
    for k in range(c.n_mb):
        sl = slice(k * c.mb, (k + 1) * c.mb)
        x = th.cat([rows(c.expert, c.e_idx[sl]), rows(c.gen, c.g_idx[sl])])
        with th.no_grad():
            if L["use_state"]:
                pn.update_stats(th.cat([c.expert["obs"][c.e_idx[sl]], c.gen["obs"][c.g_idx[sl]]]))
            rn.update_stats(x)
        logits = mlp((x - rn.running_mean) / th.sqrt(rn.running_var + rn.eps)).squeeze(1)
        loss = F.binary_cross_entropy_with_logits(logits, labels) * (c.mb / c.B)
        loss.backward()
    grads = th.cat([p.grad.reshape(-1) for p in params])
    opt.step()
    stats = compute_train_stats(logits.detach(), labels.long(), loss.detach())
    return rn, pn, grads, th.cat([p.detach().reshape(-1) for p in params]), stats


@pytest.mark.parametrize("weight_decay", [0.0, 0.01])
@pytest.mark.parametrize("warm", WARM)
@pytest.mark.parametrize("name", EAGER_CASES)
def test_reference_matches_eager_host_path(name, warm, weight_decay):
    from imitation_amd.algorithms.adversarial.common import train_stats_from_sums

    c = make_case(name, warm, weight_decay)
    ref = reference(name, warm, weight_decay)
    rn, pn, grads, params, stats = _eager_host_update(c)
    for got, want in ((rn, ref["rew_states"][-1]), (pn, ref["pol_states"][-1])):
        th.testing.assert_close(got.running_mean.double(), want["mean"], rtol=1e-5, atol=1e-5)
        th.testing.assert_close(got.running_var.double(), want["var"], rtol=1e-4, atol=1e-5)
        assert int(got.count) == want["count"]
    th.testing.assert_close(grads.double(), ref["grads"], rtol=1e-5, atol=1e-6)
    th.testing.assert_close(params.double(), ref["params"], rtol=1e-5, atol=1e-6)
    s, rows = ref["stats"].tolist(), 2 * c.mb
    want = train_stats_from_sums([s[0] / rows * (c.mb / c.B), s[1] / rows, float(c.mb), s[2], s[3], s[4], s[5] / rows],
                                 float(rows))
    for k in ("disc_loss", "disc_entropy"):
        assert stats[k] == pytest.approx(want[k], rel=1e-5, abs=1e-6)
    for k in ("disc_acc", "disc_acc_expert", "disc_acc_gen", "disc_proportion_expert_pred", "n_expert", "n_generated"):
        assert stats[k] == pytest.approx(want[k], rel=1e-6), k  # ratios of exactly equal counts


@pytest.mark.parametrize("warm", WARM)
@pytest.mark.parametrize("name", CASE_NAMES)
def test_reference_conditions(name, warm):
    """What make_case promises about the inputs, checked on the two reference modes alone: no
    hidden ReLU unit changes sign under bf16 rounding (with a margin of 4), at most 1% of the
    last minibatch's logits are close enough to 0 to, and the bf16-operand mode itself is
    inside the gradient, loss and entropy bounds the kernel is held to."""
    c = make_case(name, warm)
    r, b = reference(name, warm), reference(name, warm, bf16=True)
    if c.act == "relu":
        for zs, zbs in zip(r["preacts"], b["preacts"]):
            for z, zb in zip(zs, zbs):
                assert float(z.abs().min()) > 4.0 * float((z - zb).abs().max())
                frac_on = float((z > 0).double().mean())
                assert 0.2 < frac_on < 0.8
    tau, n_tau = logit_tau(name, warm)
    assert n_tau <= 0.01 * 2 * c.mb, (tau, n_tau)
    g, gb = r["grads"], b["grads"]
    bound = 2e-2 * g.abs() + 2.5e-3 * float(g.abs().max())
    assert float(((gb - g).abs() / bound).max()) < 0.75
    for x, xb in zip(stats_to_logged(r["stats"], c), stats_to_logged(b["stats"], c)):  # loss, entropy
        assert abs(x - xb) < 0.8 * 2e-3 * max(1.0, abs(x))


def test_reference_bf16_mode_rounds_operands():
    """The bf16-operand mode differs from float64 by about 2^-9 per operand, not by nothing
    and not by much more."""
    g, gb = reference("two_wave")["grads"], reference("two_wave", bf16=True)["grads"]
    rel = float((gb - g).norm() / g.norm())
    assert 1e-4 < rel < 2e-2, rel


def test_reference_uses_last_minibatch_stats_and_sums_gradients():
    c = make_case("three_mb")
    ref = reference("three_mb")
    assert len(ref["X"]) == len(ref["logits"]) == 3
    assert [s["count"] for s in ref["rew_states"]] == [2 * c.mb, 4 * c.mb, 6 * c.mb]
    z = ref["logits"][-1]
    assert float(ref["stats"][2]) == float((z < 0).sum())
    # minibatches have distinct rows, and X is [expert ; generator] in the s | a layout
    assert not th.equal(ref["X"][0], ref["X"][1])
    k, mb = 1, c.mb
    th.testing.assert_close(ref["X"][k][0, :17], c.expert["obs"][c.e_idx[k * mb]].double(), rtol=0, atol=0)
    th.testing.assert_close(ref["X"][k][mb, 17:], c.gen["acts"][c.g_idx[k * mb]].double(), rtol=0, atol=0)


def _native():
    from imitation_amd import _native as nat

    return nat.load()


@pytest.mark.parametrize("name", CASE_NAMES)
def test_disc_plan_sizes_follow_the_launch_geometry(name):
    D, _, _, _, _, B, mb, waves = CASES[name]
    _, dims = _layout(name)
    gblk, fblk, n_params = _native().disc_plan_sizes(dims, mb)
    assert gblk == -(-2 * mb // 64)
    assert fblk == -(-2 * mb // (16 * waves))
    assert n_params == sum(o * i + o for i, o in zip(dims[:-1], dims[1:]))


@pytest.mark.parametrize("dims,waves", [([23, 96, 1], 4), ([128, 1], 4), ([23, 128, 1], 2), ([128, 32, 1], 2),
                                        ([23, 128, 128, 1], 2), ([23, 32, 32, 1], 4)])
def test_wave_choice_counts_the_static_lds(dims, waves):
    """4 waves whenever image + static scratch fit 160 KiB: only the exact-fit two-layer
    128-wide image moved to 2 waves, its neighbours keep theirs."""
    pad32 = lambda x: (x + 31) // 32 * 32  # noqa: E731
    dm, L, rows = pad32(max(dims)), len(dims) - 1, 64
    w, h, ht = dm * (dm + 8) * 2, rows * (dm + 8) * 2, dm * (rows + 8) * 2
    image4 = w + L * h + ht + 2 * (h + ht) + 2 * 4 * dm * 4  # plan_tmlp(d, 4).bwd_lds
    static4 = 4 * 8 * 4                                      # disc_st[4][kDiscStats]
    assert (image4 + static4 <= 160 * 1024) == (waves == 4)
    assert _native().disc_plan_sizes(dims, 64)[1] == -(-128 // (16 * waves))


# ------------------------------------------------------------------ GPU: the plan, launch by launch


class DevCase:
    """The tensors ``DeviceGAIL._setup_fused_disc`` hands to ``DiscPlan``, from a CPU case.
    Workspaces start as NaN: everything the plan reads it must have written."""

    def __init__(self, c, no_rew=False, slab_short=0, partials_short=0):
        C = _native()
        dev = th.device("cuda")
        self.c = c
        L, dims = c.layout, c.dims
        gblk, fblk, n = C.disc_plan_sizes(dims, c.mb)
        assert n == c.n_params
        self.fblk = fblk
        self.flat = th.cat([t.reshape(-1) for pair in zip(c.Ws, c.bs) for t in pair]).to(dev)
        W, b, off = [], [], 0
        for Wl, bl in zip(c.Ws, c.bs):
            W.append(self.flat[off:off + Wl.numel()].view_as(Wl))
            off += Wl.numel()
            b.append(self.flat[off:off + bl.numel()])
            off += bl.numel()
        self.m, self.v = c.adam["exp_avg"].to(dev), c.adam["exp_avg_sq"].to(dev)

        def norm(state):
            return dict(mean=state["mean"].to(dev), var=state["var"].to(dev),
                        count=th.tensor(state["count"], dtype=th.int32, device=dev))

        self.rew = None if no_rew else norm(c.rew)
        # the trainer only takes a policy norm next to a reward net that sees the state
        self.pol = norm(c.pol) if L["use_state"] else None
        nan = lambda *sh: th.full(sh, float("nan"), device=dev)  # noqa: E731
        self.ws = dict(X=nan(2 * c.mb, dims[0]), partials=nan(C.disc_partials_floats(c.mb, dims[0]) - partials_short),
                       slab=nan(c.n_mb * fblk * n - slab_short), stats_slab=nan(c.n_mb * fblk * 8), grads=nan(n),
                       sums=th.zeros(2 * dims[0], device=dev, dtype=th.float64))
        src = {}
        for tag, s in (("e", c.expert), ("g", c.gen)):
            for k in ("obs", "next_obs", "acts", "dones"):
                src[f"{tag}_{k}"] = s[k].to(dev).contiguous()
        self.src = src
        rew, pol = self.rew, self.pol
        self.args = dict(batch=c.B, minibatch=c.mb, W=W, b=b, hidden_act=ACT_CODE[c.act],
                         rew_mean=rew["mean"] if rew else None, rew_var=rew["var"] if rew else None,
                         rew_count=rew["count"] if rew else None, rew_eps=REW_EPS,
                         pol_mean=pol["mean"] if pol else None, pol_var=pol["var"] if pol else None,
                         pol_count=pol["count"] if pol else None, params=self.flat, exp_avg=self.m, exp_avg_sq=self.v, beta1=BETA1, beta2=BETA2, eps=ADAM_EPS,
                         weight_decay=c.adam["weight_decay"], **L, **src, **self.ws)
        self.e_idx, self.g_idx = c.e_idx.to(dev), c.g_idx.to(dev)
        self.stats = th.full((8,), float("nan"), device=dev)
        self.plan = C.DiscPlan(self.args)

    @staticmethod
    def _norm_cpu(s):
        return None if s is None else dict(mean=s["mean"].cpu().clone(), var=s["var"].cpu().clone(), count=int(s["count"]))

    def norms(self):
        return self._norm_cpu(self.rew), self._norm_cpu(self.pol)

    def state(self):
        """Everything an update may write, on the CPU."""
        rew, pol = self.norms()
        out = dict(params=self.flat, m=self.m, v=self.v, X=self.ws["X"], stats=self.stats)
        for tag, s in (("rew", rew), ("pol", pol)):
            if s is not None:
                out.update({f"{tag}_mean": s["mean"], f"{tag}_var": s["var"], f"{tag}_count": th.tensor(s["count"])})
        return {k: v.detach().cpu().clone() for k, v in out.items()}

    def adam_scalars(self, t):
        return LR / (1.0 - BETA1**t), (1.0 - BETA2**t) ** 0.5


def assert_norm(got, want):
    th.testing.assert_close(got["mean"].double(), want["mean"], rtol=1e-5, atol=1e-5)
    th.testing.assert_close(got["var"].double(), want["var"], rtol=1e-4, atol=1e-5)
    assert got["count"] == want["count"]


def assert_bitwise(a, b):
    assert a.keys() == b.keys()
    bad = [k for k in a if not th.equal(a[k].view(th.int32) if a[k].dtype == th.float32 else a[k],
                                        b[k].view(th.int32) if b[k].dtype == th.float32 else b[k])]
    assert not bad, bad


@functools.lru_cache(maxsize=None)
def staged(name, warm=False, weight_decay=0.0):
    """One staged pass on the GPU: gather / norm / fwd_bwd per minibatch, the reduction to
    ``grads`` and the statistics, then three Adam steps from those gradients. Snapshots on the CPU."""
    d = DevCase(make_case(name, warm, weight_decay))
    c, plan = d.c, d.plan
    out = dict(X=[], rew=[], pol=[], adam=[])
    for k in range(c.n_mb):
        plan.gather(k, d.e_idx, d.g_idx)
        out["X"].append(d.ws["X"].cpu().clone())
        plan.norm(0, 0, True, True)
        rew, pol = d.norms()
        out["rew"].append(rew)
        out["pol"].append(pol)
        plan.fwd_bwd(k)
    plan.adam(1, 0, 0.0, 1.0, d.stats)
    out["grads"], out["stats"] = d.ws["grads"].cpu().clone(), d.stats.cpu().clone()
    out["params_before_adam"] = d.flat.cpu().clone()
    for i in range(3):
        plan.adam(0, 1, *d.adam_scalars(ADAM_STEPS_TAKEN + 1 + i), None)
        out["adam"].append((d.flat.cpu().clone(), d.m.cpu().clone(), d.v.cpu().clone()))
    return out


CASE_WARM = [(n, w) for n in CASE_NAMES for w in WARM]


@gpu
@pytest.mark.parametrize("name,warm", CASE_WARM)
def test_gather_is_exact(name, warm):
    got, ref = staged(name, warm), reference(name, warm)
    for k, X in enumerate(got["X"]):
        assert th.equal(X.double(), ref["X"][k]), k


@gpu
@pytest.mark.parametrize("name,warm", CASE_WARM)
def test_norms_after_every_minibatch(name, warm):
    """Fresh and warm running norms; the off-centre and the constant column are held to the
    same tolerances as every other."""
    got, ref = staged(name, warm), reference(name, warm)
    c = make_case(name, warm)
    for k in range(c.n_mb):
        for g, r in ((got["rew"][k], ref["rew_states"][k]), (got["pol"][k], ref["pol_states"][k])):
            if g is None:
                continue
            rel = ((g["var"].double() - r["var"]).abs() / r["var"].clamp_min(1e-30)).max()
            print(f"{name} warm={warm} k={k}: max rel var err {float(rel):.3e}")
        assert_norm(got["rew"][k], ref["rew_states"][k])
        if c.layout["use_state"]:
            assert_norm(got["pol"][k], ref["pol_states"][k])


@gpu
@pytest.mark.parametrize("name,warm", CASE_WARM)
def test_gradients_against_fp64(name, warm):
    got, c = staged(name, warm), make_case(name, warm)
    # reducing to grads (adam(1, 0)) left the parameters alone
    assert th.equal(got["params_before_adam"], th.cat([t.reshape(-1) for p in zip(c.Ws, c.bs) for t in p]))
    assert_grads(got["grads"], name, warm)


@gpu
@pytest.mark.parametrize("name,warm", CASE_WARM)
def test_statistics_of_the_last_minibatch(name, warm):
    c = make_case(name, warm)
    tau, n_tau = logit_tau(name, warm)
    assert n_tau <= 0.01 * 2 * c.mb  # on the reference, before the kernel's counts are looked at
    got, ref = staged(name, warm)["stats"].double(), reference(name, warm)["stats"]
    print(f"{name} warm={warm}: stats {got.tolist()} ref {ref.tolist()} tau {tau:.4f} rows inside {n_tau}")
    for a, b in zip(stats_to_logged(got, c), stats_to_logged(ref, c)):
        assert abs(a - b) < 2e-3 * max(1.0, abs(b)), (a, b)
    for i in range(1, 5):
        assert abs(float(got[i]) - float(ref[i])) <= n_tau, (i, got.tolist(), ref.tolist())
        assert float(got[i]) == round(float(got[i]))
    assert float(got[6]) == 0.0 and float(got[7]) == 0.0


@gpu
@pytest.mark.parametrize("weight_decay", [0.0, 0.01])
@pytest.mark.parametrize("name", CASE_NAMES)
def test_adam_from_reduced_grads(name, weight_decay):
    got = staged(name, False, weight_decay)
    c = make_case(name, False, weight_decay)
    a = c.adam
    p, m, v = got["params_before_adam"].double(), a["exp_avg"].double(), a["exp_avg_sq"].double()
    for i, (gp, gm, gv) in enumerate(got["adam"]):
        p, m, v = dref.adam_step_reference(p, got["grads"], m, v, ADAM_STEPS_TAKEN + 1 + i, LR, BETA1, BETA2, ADAM_EPS,
                                           weight_decay)
        th.testing.assert_close(gp.double(), p, rtol=1e-6, atol=1e-7)
        # the moments: the kernel forms 1 - beta in fp32, which is off by up to 2^-24 / (1 - beta)
        # relative (6e-7 for beta1 = 0.9, 6e-5 for beta2 = 0.999) from the double torch casts
        th.testing.assert_close(gm.double(), m, rtol=1e-5, atol=1e-6 * float(m.abs().max()))
        th.testing.assert_close(gv.double(), v, rtol=1e-4, atol=1e-6 * float(v.abs().max()))
    if weight_decay:  # and the decay did something
        assert not th.equal(got["adam"][0][0], staged(name, False, 0.0)["adam"][0][0])


@gpu
@pytest.mark.parametrize("name", CASE_NAMES)
def test_update_is_the_staged_sequence_bitwise(name):
    c = make_case(name, True, 0.01)
    step = ADAM_STEPS_TAKEN + 1
    a = DevCase(c)
    for k in range(c.n_mb):
        a.plan.gather(k, a.e_idx, a.g_idx)
        a.plan.norm(0, 0, True, True)
        a.plan.fwd_bwd(k)
    a.plan.adam(1, 0, 0.0, 1.0, a.stats)
    a.plan.adam(0, 1, *a.adam_scalars(step), None)
    b, b2 = DevCase(c), DevCase(c)
    for d in (b, b2):
        d.plan.update(d.e_idx, d.g_idx, *d.adam_scalars(step), True, True, d.stats)
    sa, sb, sb2 = a.state(), b.state(), b2.state()
    assert not th.equal(sb["params"], th.cat([t.reshape(-1) for p in zip(c.Ws, c.bs) for t in p]))
    assert not any(bool(th.isnan(v.double()).any()) for v in sb.values())
    assert_bitwise(sb, sb2)
    assert_bitwise(sa, sb)


# ------------------------------------------------------------------ GPU: checked once


@gpu
@pytest.mark.parametrize("merge_rew,merge_pol", [(False, True), (True, False)])
def test_merge_flags_leave_that_norm_alone(merge_rew, merge_pol):
    name = "three_mb"
    c = make_case(name, True)
    ref = reference(name, True, merge_rew=merge_rew, merge_pol=merge_pol)
    d = DevCase(c)
    rew0, pol0 = d.norms()
    for k in range(c.n_mb):
        d.plan.gather(k, d.e_idx, d.g_idx)
        d.plan.norm(0, 0, merge_rew, merge_pol)
        d.plan.fwd_bwd(k)
    d.plan.adam(1, 0, 0.0, 1.0, d.stats)
    rew, pol = d.norms()
    for flag, before, after, want in ((merge_rew, rew0, rew, ref["rew_states"][-1]), (merge_pol, pol0, pol, ref["pol_states"][-1])):
        if flag:
            assert_norm(after, want)
        else:
            assert th.equal(before["mean"], after["mean"]) and th.equal(before["var"], after["var"])
            assert before["count"] == after["count"] == 5000
    # normalised with the state as the flags left it
    assert_grads(d.ws["grads"], name, True, merge_rew=merge_rew, merge_pol=merge_pol)


@gpu
def test_plan_without_reward_normaliser():
    """No running mean to shift the moment sums by, an un-normalised input with a column near
    100: the policy norm still matches, and the gradients are those of the raw input."""
    name = "baseline"
    c = make_case(name)
    ref = reference(name, no_rew=True)
    d = DevCase(c, no_rew=True)
    d.plan.gather(0, d.e_idx, d.g_idx)
    d.plan.norm(0, 0, True, True)
    d.plan.fwd_bwd(0)
    d.plan.adam(1, 0, 0.0, 1.0, d.stats)
    assert th.equal(d.ws["X"].cpu().double(), ref["X"][0])
    _, pol = d.norms()
    assert_norm(pol, ref["pol_states"][0])
    (emax, el2), (bmax, bl2) = grad_errors(d.ws["grads"], name, False, no_rew=True)
    print(f"no reward norm: kernel err max {emax:.3e} l2 {el2:.3e}; bf16 mode {bmax:.3e} {bl2:.3e}")
    assert emax <= 4.0 * bmax and el2 <= 4.0 * bl2


@gpu
def test_deferred_policy_merge_is_the_in_place_merge():
    name = "three_mb"
    c = make_case(name, True)
    ref = reference(name, True)
    a, b = DevCase(c), DevCase(c)
    D = c.layout["obs_dim"]
    assert b.plan.pol_cols == D and b.plan.n_minibatches == c.n_mb
    buf = th.full((c.n_mb, 2 * D + 1), float("nan"), device="cuda")
    b.plan.set_pol_defer(buf)
    _, pol0 = b.norms()
    for k in range(c.n_mb):
        a.plan.gather(k, a.e_idx, a.g_idx)
        a.plan.norm(0, 0, True, True)
        b.plan.gather(k, b.e_idx, b.g_idx)
        b.plan.norm(0, 0, True, True, k)
    rew_a, pol_a = a.norms()
    rew_b, pol_b = b.norms()
    assert th.equal(pol_b["mean"], pol0["mean"]) and th.equal(pol_b["var"], pol0["var"]) and pol_b["count"] == 5000
    assert th.equal(rew_a["mean"], rew_b["mean"]) and th.equal(rew_a["var"], rew_b["var"])
    rec = buf.cpu().double()
    for k in range(c.n_mb):
        bmean, bvar = dref.batch_moments(ref["X"][k][:, :D])
        th.testing.assert_close(rec[k, :D], bmean, rtol=1e-5, atol=1e-5)
        th.testing.assert_close(rec[k, D:2 * D], bvar, rtol=1e-4, atol=1e-5)
        assert float(rec[k, 2 * D]) == 2 * c.mb
    b.plan.pol_norm_merge(c.n_mb)
    _, pol_b = b.norms()
    assert th.equal(pol_a["mean"], pol_b["mean"]) and th.equal(pol_a["var"], pol_b["var"])
    assert pol_a["count"] == pol_b["count"] == 5000 + 2 * c.B


@gpu
@pytest.mark.parametrize("warm", WARM)
def test_data_parallel_norm_modes_in_one_process(warm):
    """Mode 1 writes the float64 moment sums and touches no norm; mode 2 merges from (all-reduced)
    sums. Two ranks with the same minibatch: the sums double, the batch is the minibatch twice."""
    name = "baseline"
    c = make_case(name, warm)
    ref = reference(name, warm)
    d = DevCase(c)
    rew0, pol0 = d.norms()
    d.plan.gather(0, d.e_idx, d.g_idx)
    d.plan.norm(1, 0, True, True)
    rew1, pol1 = d.norms()
    for x, y in ((rew0, rew1), (pol0, pol1)):
        assert th.equal(x["mean"], y["mean"]) and th.equal(x["var"], y["var"]) and x["count"] == y["count"]
    X = ref["X"][0]
    din = c.dims[0]
    shift = rew0["mean"].double()  # the shift every rank agrees on: the running mean
    sums = d.ws["sums"].cpu()
    th.testing.assert_close(sums[:din], (X - shift).sum(0), rtol=1e-5, atol=1e-3)
    th.testing.assert_close(sums[din:], ((X - shift) ** 2).sum(0), rtol=1e-4, atol=1e-3)
    d.ws["sums"].mul_(2.0)
    d.plan.norm(2, 4 * c.mb, True, True)
    X2 = th.cat([X, X])
    bmean, bvar = dref.batch_moments(X2)
    want_rew = dref.chan_merge(dref.norm_state(c.rew), bmean, bvar, 4 * c.mb)
    want_pol = dref.chan_merge(dref.norm_state(c.pol), bmean[:17], bvar[:17], 4 * c.mb)
    rew2, pol2 = d.norms()
    if warm:  # with a running mean near the data the sums are well conditioned
        assert_norm(rew2, want_rew)
        assert_norm(pol2, want_pol)
    else:
        # Documented limitation of the DP modes (disc.hip): the shift is the running mean, which
        # is 0 here, so the column near 100 keeps fp32's cancellation error in its variance.
        well = th.ones(din, dtype=th.bool)
        well[0] = False
        for got, want, m in ((rew2, want_rew, well), (pol2, want_pol, well[:17])):
            assert_norm({k: (v[m] if k != "count" else v) for k, v in got.items()},
                        {k: (v[m] if k != "count" else v) for k, v in want.items()})
            th.testing.assert_close(got["mean"].double(), want["mean"], rtol=1e-5, atol=1e-5)
            th.testing.assert_close(got["var"].double(), want["var"], rtol=1e-2, atol=1e-5)


@gpu
def test_input_wider_than_128_is_refused():
    C = _native()
    dev = th.device("cuda")
    D, A, rows = 60, 9, 8
    din = 2 * D + A
    assert din == 129
    X = th.full((2 * 4, din), -7.0, device=dev)
    flat = th.zeros(din * 32 + 32 + 32 + 1, device=dev)
    W = [flat[:din * 32].view(32, din), flat[din * 32 + 32:din * 32 + 64].view(1, 32)]
    b = [flat[din * 32:din * 32 + 32], flat[din * 32 + 64:]]
    z = lambda *sh, dt=th.float32: th.zeros(*sh, device=dev, dtype=dt)  # noqa: E731
    src = {f"{t}_{k}": v for t in "eg" for k, v in (("obs", z(rows, D)), ("next_obs", z(rows, D)), ("acts", z(rows, A)),
                                                   ("dones", z(rows, dt=th.bool)))}
    args = dict(batch=4, minibatch=4, W=W, b=b, hidden_act=1, rew_mean=z(din), rew_var=z(din) + 1,
                rew_count=z((), dt=th.int32), rew_eps=REW_EPS, obs_dim=D, act_width=A, use_state=1, use_action=1,
                use_next_state=1, use_done=0, act_discrete=0, pol_mean=z(D), pol_var=z(D) + 1, pol_count=z((), dt=th.int32),
                params=flat, exp_avg=z(flat.numel()), exp_avg_sq=z(flat.numel()), beta1=BETA1, beta2=BETA2, eps=ADAM_EPS,
                weight_decay=0.0, X=X, partials=z(C.disc_partials_floats(4, din)), slab=z(4 * flat.numel()), stats_slab=z(4 * 8),
                grads=z(flat.numel()), sums=z(2 * din, dt=th.float64), **src)
    idx = th.zeros(4, dtype=th.int64, device=dev)
    with pytest.raises(RuntimeError):
        plan = C.DiscPlan(args)
        plan.gather(0, idx, idx)
    th.cuda.synchronize()
    assert bool((X == -7.0).all())


@gpu
@pytest.mark.parametrize("short", ["slab", "partials"])
def test_short_workspace_is_refused_at_construction(short):
    with pytest.raises(RuntimeError, match="too small"):
        DevCase(make_case("three_mb"), **{f"{short}_short": 1})
