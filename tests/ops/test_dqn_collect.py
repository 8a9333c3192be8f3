"""The device-resident DQN collection kernel (``imitation_amd.ops.dqn.dqn_collect``;
``csrc/kernels/dqn_collect.hip``) against ``dqn_collect_reference`` (torch Q, the recorded
actions through ``dagger_env_step``), the Python ``splitmix64`` mirror and an fp64 Q."""

import numpy as np
import pytest
import torch as th

from imitation_amd.ops import dqn as td

pytestmark = pytest.mark.gpu

ALWAYS, HALF = td.EXPLORE_ALWAYS, 1 << 23
# name -> env, hidden widths, N, K, launches, max_steps (None: the env's), ring slots S, thresholds of a launch
SHAPES = {
    # CartPole-v1 terminates: all-explore actions (known from the stream alone) end an episode in 48 steps
    "a": dict(env="CartPole-v1", net=(64, 64), N=1, K=4, launches=12, max_steps=None, S=64, thr=[ALWAYS] * 4),
    # TimeLimit of 3 and a ring of 4 slots: truncations, a wrap inside a launch (K > S) and across launches
    "b": dict(env="MountainCar-v0", net=(24, 40), N=3, K=5, launches=3, max_steps=3, S=4,
              thr=[HALF, 0, ALWAYS, HALF + 12345, HALF]),
    # 17 workgroups of 4 waves, the last one with a single env
    "c": dict(env="Acrobot-v1", net=(64, 64), N=65, K=16, launches=2, max_steps=None, S=40, thr=[HALF] * 15 + [HALF // 2]),
    "d": dict(env="seals/CartPole-v0", net=(1, 1), N=1, K=1, launches=1, max_steps=None, S=2, thr=[0]),  # (its one step is greedy)
}
ENV_SEED, ACT_SEED, NET_SEED = 3, 11, 5
MODES = {"dqn": dict(reward_const=None, write_timeouts=True), "sqil": dict(reward_const=0.0, write_timeouts=False)}
ENV_KEYS = ("state", "rng", "elapsed", "ep_ret", "cur_obs")


def make_inputs(shape, dev="cuda", net=None, thr=None):
    from imitation_amd.envs.vec_env import NativeVecEnv

    s = SHAPES[shape]
    venv = NativeVecEnv(s["env"], s["N"], seed=ENV_SEED, max_episode_steps=s["max_steps"])
    obs0 = venv.reset()
    st = venv.get_state()
    N = s["N"]
    D, A = int(np.prod(venv.observation_space.shape)), int(venv.action_space.n)
    env = dict(env=s["env"], max_steps=int(venv.max_episode_steps),
               state=th.as_tensor(st["state"], device=dev).float().contiguous(),
               rng=th.as_tensor(st["rng"].astype(np.int64), device=dev).contiguous(),
               elapsed=th.as_tensor(st["elapsed"].astype(np.int32), device=dev).contiguous(),
               ep_ret=th.zeros(N, device=dev),
               cur_obs=th.as_tensor(np.asarray(obs0, np.float32), device=dev).reshape(N, D).contiguous())
    H1, H2 = net or s["net"]
    L = td.TDLayout.from_dims(D, H1, H2, A)
    gen = th.Generator().manual_seed(NET_SEED)
    flat = th.zeros(L.n + (-L.n) % 4)
    for v in L.views(flat):  # nn.Linear's default range
        k = v.shape[-1] if v.dim() == 2 else max(v.numel(), 1)
        v.copy_((th.rand(v.shape, generator=gen) * 2 - 1) / np.sqrt(k))
    SN = s["S"] * N
    ring = [th.zeros(SN, D, device=dev), th.zeros(SN, D, device=dev), th.zeros(SN, 1, dtype=th.int64, device=dev),
            th.zeros(SN, device=dev), th.zeros(SN, device=dev), th.zeros(SN, device=dev)]
    return dict(s, shape=shape, env_block=env, L=L, flat=flat.to(dev), ring=ring, D=D, A=A,
                act_rng=td.action_streams(ACT_SEED, N, dev), thr=list(thr or s["thr"]))


def clone_inputs(c):
    out = dict(c)
    out["env_block"] = {k: (v.clone() if isinstance(v, th.Tensor) else v) for k, v in c["env_block"].items()}
    out["ring"] = [t.clone() for t in c["ring"]]
    out["act_rng"] = c["act_rng"].clone()
    return out


def run_kernel(c, mode):
    """Every launch of the case: the per-launch records (with the explore flags and q)."""
    recs, pos = [], 0
    err = th.zeros(1, dtype=th.int32, device="cuda")
    for _ in range(c["launches"]):
        rec = td.collect_records(c["K"], c["N"], c["A"], "cuda", explore=True, q=True)
        td.dqn_collect(c["env_block"], c["ring"], pos, c["S"], c["flat"], c["L"], c["thr"], c["act_rng"], records=rec,
                       err=err, **MODES[mode])
        recs.append(rec)
        pos = (pos + c["K"]) % c["S"]
    assert int(err.item()) == 0
    return recs


def run_reference(c, mode, actions):
    recs, pos = [], 0
    for a in actions:
        rec = td.collect_records(c["K"], c["N"], c["A"], "cuda", q=True)
        rec["obs"] = th.zeros(c["K"], c["N"], c["D"], device="cuda")
        td.dqn_collect_reference(c["env_block"], c["ring"], pos, c["S"], c["flat"], c["L"], a, records=rec, **MODES[mode])
        recs.append(rec)
        pos = (pos + c["K"]) % c["S"]
    return recs


_CACHE = {}


def both(shape, mode):
    """The kernel run and the reference replay of its actions, computed once per (shape, mode)."""
    if (shape, mode) not in _CACHE:
        k = make_inputs(shape)
        r = clone_inputs(k)
        init = clone_inputs(k)
        k_recs = run_kernel(k, mode)
        r_recs = run_reference(r, mode, [rec["action"] for rec in k_recs])
        _CACHE[shape, mode] = (init, k, k_recs, r, r_recs)
    return _CACHE[shape, mode]


def mirror_draws(c):
    """The documented action stream of every env over all launches, in Python ints:
    (flags [launches, K, N], random actions (-1: greedy), final states [N])."""
    flags = np.zeros((c["launches"], c["K"], c["N"]), dtype=np.int64)
    acts = -np.ones((c["launches"], c["K"], c["N"]), dtype=np.int64)
    states = []
    for n in range(c["N"]):
        s = td.seed_stream(ACT_SEED, n)
        for l in range(c["launches"]):
            f, a, s = td.explore_draws(s, c["thr"], c["A"])
            flags[l, :, n] = f
            acts[l, :, n] = [-1 if x is None else x for x in a]
        states.append(s)
    return flags, acts, states


@pytest.mark.parametrize("mode", list(MODES))
@pytest.mark.parametrize("shape", list(SHAPES))
def test_bitwise_replay(shape, mode):
    init, k, k_recs, r, r_recs = both(shape, mode)
    for key in ENV_KEYS:
        assert th.equal(k["env_block"][key], r["env_block"][key]), key
    for name, a, b in zip(("obs", "next_obs", "actions", "rewards", "dones", "timeouts"), k["ring"], r["ring"]):
        assert th.equal(a, b), name
    for kr, rr in zip(k_recs, r_recs):
        for key in ("done", "ep_ret", "ep_len"):
            assert th.equal(kr[key], rr[key]), key
    # the events this case is there for, counted on the reference's outputs alone
    ref_done = th.stack([rr["done"] for rr in r_recs])  # [launches, K, N]
    flags, _, _ = mirror_draws(k)
    if shape == "a":  # max_steps 500: an episode that ends within 48 steps has terminated
        assert k["env_block"]["max_steps"] == 500 and k["launches"] * k["K"] < 500
        assert int(ref_done.sum()) >= 1
        assert flags.all()
    if shape == "b":  # MountainCar never reaches the goal in 3 steps: every done is a truncation
        assert int(ref_done.sum()) >= 3 * k["N"]
        assert k["K"] > k["S"] and k["launches"] * k["K"] > 2 * k["S"]  # wraps inside a launch and across launches
        assert (k["K"] % k["S"]) != 0  # later launches start inside the ring
        if mode == "dqn":
            assert int(r["ring"][5].sum()) >= 1 and th.equal(r["ring"][5], r["ring"][4])
    if shape in ("b", "c"):
        assert flags.any() and not flags.all()
    if mode == "sqil":
        assert float(r["ring"][3].abs().max()) == 0.0 and float(k["ring"][3].abs().max()) == 0.0
        assert float(r["ring"][5].abs().max()) == 0.0 and float(k["ring"][5].abs().max()) == 0.0
        if shape == "b":  # the newest slot of env 0 is step 14: elapsed 3, truncated, stored as done
            last = ((k["launches"] * k["K"] - 1) % k["S"]) * k["N"]
            assert float(r["ring"][4][last]) == 1.0 and float(k["ring"][4][last]) == 1.0
    else:  # the env reward (every env here pays +-1 per step)
        assert float(r["ring"][3].abs().max()) == 1.0


@pytest.mark.parametrize("shape", ["b", "c"])
def test_exploration_is_the_documented_stream(shape):
    init, k, k_recs, _, _ = both(shape, "dqn")
    flags, acts, states = mirror_draws(k)
    for l, rec in enumerate(k_recs):
        ex = rec["explore"].cpu().numpy()
        assert np.array_equal(ex, flags[l])
        a = rec["action"].cpu().numpy()
        assert np.array_equal(a[ex == 1], acts[l][ex == 1])
    assert td.stream_states(k["act_rng"]) == states


@pytest.mark.parametrize("thr,explores", [(0, False), (ALWAYS, True)])
def test_threshold_ends(thr, explores):
    c = make_inputs("b", thr=[thr] * 5)
    c["launches"] = 1
    rec = run_kernel(c, "dqn")[0]
    flags, acts, states = mirror_draws(c)
    assert bool(flags.all()) == explores and bool(flags.any()) == explores
    assert np.array_equal(rec["explore"].cpu().numpy(), flags[0])
    got = td.stream_states(c["act_rng"])
    assert got == states
    for n in range(c["N"]):  # one draw per greedy step, two per explored one
        s = td.seed_stream(ACT_SEED, n)
        for _ in range(c["K"] * (2 if explores else 1)):
            s, _ = td.splitmix64(s)
        assert got[n] == s
    if explores:
        assert np.array_equal(rec["action"].cpu().numpy(), acts[0])


def _ulp(x: float) -> float:
    return float(np.spacing(np.float32(abs(x))))


@pytest.mark.parametrize("shape", list(SHAPES))
def test_greedy_action_and_q_numerics(shape):
    """Greedy steps take the lowest index of the maximum of the kernel's own q (exact); q against
    fp64 within the bound of tests/ops/test_dqn_td.py: 4 x the error of fp32 torch eager on the
    same inputs plus one fp32 ulp of the largest |q|."""
    init, k, k_recs, r, r_recs = both(shape, "dqn")
    q = th.stack([rec["q"] for rec in k_recs])  # [launches, K, N, A]
    act = th.stack([rec["action"] for rec in k_recs])
    ex = th.stack([rec["explore"] for rec in k_recs])
    A = k["A"]
    idx = th.arange(A, device=q.device).expand_as(q)
    lowest = th.where(q == q.max(dim=-1, keepdim=True).values, idx, th.full_like(idx, A)).min(dim=-1).values
    greedy = ex == 0
    if shape != "a":
        assert int(greedy.sum()) > 0
    assert th.equal(act[greedy], lowest[greedy])
    obs = th.stack([rr["obs"] for rr in r_recs])
    q64 = td.q_values(obs.double(), k["flat"].double(), k["L"])
    q32 = th.stack([rr["q"] for rr in r_recs])
    err_k = float((q.double() - q64).abs().max())
    err_e = float((q32.double() - q64).abs().max())
    bound = 4 * err_e + _ulp(float(q64.abs().max()))
    print(f"dqn_collect {shape} q: kernel {err_k:.3e} eager {err_e:.3e} "
          f"ratio {err_k / err_e if err_e else float('inf'):.2f} bound {bound:.3e} ({err_k / bound:.2f} of it)")
    assert err_k <= bound


@pytest.mark.parametrize("shape", ["b", "c"])
def test_bitwise_repeatable(shape):
    a = make_inputs(shape)
    b = clone_inputs(a)
    ra, rb = run_kernel(a, "dqn"), run_kernel(b, "dqn")
    for key in ENV_KEYS:
        assert th.equal(a["env_block"][key], b["env_block"][key])
    assert th.equal(a["act_rng"], b["act_rng"])
    for x, y in zip(a["ring"], b["ring"]):
        assert th.equal(x, y)
    for x, y in zip(ra, rb):
        for key in x:
            assert th.equal(x[key], y[key]), key


@pytest.mark.parametrize("bad", [float("nan"), float("inf")])
def test_non_finite_q_sets_the_error_word_and_acts_zero(bad):
    c = make_inputs("b", thr=[0] * 5)
    c["L"].views(c["flat"])[5][1] = bad  # b3[1]: one Q-value of every env
    err = th.zeros(1, dtype=th.int32, device="cuda")
    rec = td.dqn_collect(c["env_block"], c["ring"], 0, c["S"], c["flat"], c["L"], c["thr"], c["act_rng"], err=err)
    assert int(err.item()) == 1
    assert int(rec["action"].abs().max()) == 0
    # a healthy launch leaves the word as it is: it persists until the host clears it
    ok = make_inputs("b", thr=[0] * 5)
    td.dqn_collect(ok["env_block"], ok["ring"], 0, ok["S"], ok["flat"], ok["L"], ok["thr"], ok["act_rng"], err=err)
    assert int(err.item()) == 1


def test_shape_limits_raise_and_launch_nothing():
    c = make_inputs("a")
    before = clone_inputs(c)
    c["thr"] = [0] * 17  # K = 17
    with pytest.raises(RuntimeError, match="dqn_collect"):
        run_kernel(dict(c, launches=1, K=17), "dqn")
    # D = 65: consistent tensors of an over-wide observation
    D = 65
    L = td.TDLayout.from_dims(D, 64, 64, c["A"])
    wide = dict(c, thr=[0] * 4, K=4, launches=1, L=L, D=D, flat=th.zeros(L.n, device="cuda"),
                env_block=dict(c["env_block"], cur_obs=th.zeros(c["N"], D, device="cuda")),
                ring=[th.zeros(c["S"], D, device="cuda"), th.zeros(c["S"], D, device="cuda")] + c["ring"][2:])
    with pytest.raises(RuntimeError, match="dqn_collect"):
        run_kernel(wide, "dqn")
    th.cuda.synchronize()
    for key in ENV_KEYS:
        assert th.equal(c["env_block"][key], before["env_block"][key])
    assert th.equal(c["act_rng"], before["act_rng"])
    for x, y in zip(c["ring"], before["ring"]):
        assert th.equal(x, y)
