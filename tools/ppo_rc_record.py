"""Record what one register-chained PPO update (csrc/kernels/ppo_rc_kernel.h) leaves behind.

For every case of ``CASES`` a trainer is built from a seeded state the way
tests/engine/test_ppo_rc_lean.py builds its trainers, one rollout and ONE ``_ppo_update`` run, and
the SHA-256 of everything the update writes is taken: the policy / value parameters, ``exp_avg``,
``exp_avg_sq``, the Adam step, the normaliser's mean / var / count and the five PPO statistics.

    python tools/ppo_rc_record.py            # writes tests/golden/ppo_rc_update_digests.json
    python tools/ppo_rc_record.py --out FILE

Only existing bindings are used, so the recorder runs unchanged on any earlier commit: the
committed JSON was recorded with the build of the commit BEFORE a kernel change, and
tests/engine/test_ppo_rc_parent_digests.py recomputes the digests on the current build. The
cases are the smallest shapes at which a piece of the per-minibatch code can go wrong: K = 1, 2,
3 and 5 minibatches (prologue and steady-state Chan merges of the normaliser), lean and full
rows, two chunks, two row groups (exchange), a run-time chunk width with A = 1, a categorical
head (no log-std), a 64-wide ReLU net without operand prefetch, a policy without normaliser, and
one case on each of the other net-split [64, 64] rows that compile the same per-minibatch code.
"""

import argparse
import hashlib
import json
import os
import sys

import numpy as np
import torch as th

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

GOLDEN = os.path.join(ROOT, "tests", "golden", "ppo_rc_update_digests.json")

_CHEETAH = "seals/HalfCheetah-v1"
_NS32 = "rc:g1x1x64:kt2:ns"


def _case(name, env_id, n_envs, n_steps, batch, n_epochs, path, row, rc_lean=1, gmax=0, net_arch=None, relu=True,
          normalize=True):
    return dict(name=name, env_id=env_id, n_envs=n_envs, n_steps=n_steps, batch=batch, n_epochs=n_epochs, path=path,
                row=row, rc_lean=rc_lean, gmax=gmax, net_arch=net_arch, relu=relu, normalize=normalize)


# K = n_epochs * (n_envs * n_steps) / batch minibatches per update
CASES = []
for _lean, _row in ((1, "ns_cheetah32_lean"), (0, "ns_cheetah32")):
    _tag = "lean" if _lean else "full"
    CASES += [
        _case(f"cheetah_{_tag}_k1", _CHEETAH, 4, 16, 64, 1, _NS32, _row, rc_lean=_lean),
        _case(f"cheetah_{_tag}_k2", _CHEETAH, 4, 16, 64, 2, _NS32, _row, rc_lean=_lean),
        _case(f"cheetah_{_tag}_k3", _CHEETAH, 4, 16, 64, 3, _NS32, _row, rc_lean=_lean),
        _case(f"cheetah_{_tag}_k5", _CHEETAH, 4, 80, 64, 1, _NS32, _row, rc_lean=_lean),
    ]
CASES += [
    # two chunks per minibatch in one row group / two row groups (partial exchange), K = 2
    _case("cheetah_b128_two_chunks_k2", _CHEETAH, 8, 32, 128, 1, "rc:g1x2x64:kt2:ns", "ns_cheetah32_lean", gmax=1),
    _case("cheetah_b128_two_groups_k2", _CHEETAH, 8, 32, 128, 1, "rc:g2x1x64:kt2:ns", "ns_cheetah32"),
    # A = 1, run-time chunk width, both nets in one workgroup
    _case("pendulum_b32_k3", "Pendulum-v1", 4, 24, 32, 1, "rc:g1x1x32:kt2", "narrow32"),
    # categorical head: no log-std vector, no entropy sum
    _case("cartpole_k3", "seals/CartPole-v0", 4, 16, 64, 3, _NS32, "ns_cartpole32_lean"),
    # 64-wide ReLU nets (KT == 4: fp32 chains, no operand prefetch)
    _case("hopper64_relu_k3", "seals/Hopper-v1", 4, 16, 64, 3, "rc:g1x1x64:kt4:ns", "ns_hopper64r_lean",
          net_arch=dict(pi=[64, 64], vf=[64, 64])),
    # policy without observation normaliser (has_norm == 0)
    _case("cheetah_no_norm_k2", _CHEETAH, 4, 16, 64, 2, _NS32, "ns_cheetah32_lean", normalize=False),
]
# the other net-split [64, 64] builds (they share the per-minibatch code of the rows above): the
# Walker2d exact row and one family row per obs-dim bound / activation / head
_W64 = dict(pi=[64, 64], vf=[64, 64])
CASES += [
    _case("walker64_relu_k3", "seals/Walker2d-v1", 4, 16, 64, 3, "rc:g1x1x64:kt4:ns", "ns_walker64r_lean", net_arch=_W64),
    _case("cheetah64_tanh_k3", _CHEETAH, 4, 16, 64, 3, "rc:g1x1x64:kt4:ns", "ns_64_d32_tanh_gauss", net_arch=_W64, relu=False),
    _case("hopper64_tanh_k3", "seals/Hopper-v1", 4, 16, 64, 3, "rc:g1x1x64:kt4:ns", "ns_64_d16_tanh_gauss", net_arch=_W64,
          relu=False),
    _case("cartpole64_relu_k3", "seals/CartPole-v0", 4, 16, 64, 3, "rc:g1x1x64:kt4:ns", "ns_64_d16_relu_cat", net_arch=_W64),
]


def build_trainer(case, seed=0):
    """tests/engine/test_device_engine.py ``_setup`` with the case's shape (and, for the case
    without normaliser, the default features extractor)."""
    from imitation_amd.data import rollout
    from imitation_amd.engine.gail import DeviceGAIL
    from imitation_amd.policies.base import FeedForward32Policy, NormalizeFeaturesExtractor
    from imitation_amd.rewards.reward_nets import BasicRewardNet, NormalizedRewardNet
    from imitation_amd.rl.policies import ActorCriticPolicy
    from imitation_amd.rl.ppo import PPO
    from imitation_amd.util import logger
    from imitation_amd.util.networks import RunningNorm
    from imitation_amd.util.util import make_vec_env

    th.manual_seed(seed)
    np.random.seed(seed)
    rng = np.random.default_rng(seed)
    env_id = case["env_id"]
    venv = make_vec_env(env_id, rng=rng, n_envs=case["n_envs"])
    demo_env = make_vec_env(env_id, rng=np.random.default_rng(7), n_envs=4)
    demo_env.action_space.seed(7)
    demos = rollout.flatten_trajectories(rollout.generate_trajectories(None, demo_env, rollout.make_min_timesteps(1024), rng=rng))
    pk = {}
    if case["normalize"]:
        pk["features_extractor_class"] = NormalizeFeaturesExtractor
    policy_cls = FeedForward32Policy
    if case["net_arch"] is not None:
        pk["net_arch"] = case["net_arch"]
        pk["activation_fn"] = th.nn.ReLU if case["relu"] else th.nn.Tanh
        policy_cls = ActorCriticPolicy
    gen = PPO(policy_cls, venv, n_steps=case["n_steps"], batch_size=case["batch"], n_epochs=case["n_epochs"], device="cuda",
              seed=seed, ent_coef=0.01, policy_kwargs=pk)
    rn = NormalizedRewardNet(BasicRewardNet(venv.observation_space, venv.action_space, normalize_input_layer=RunningNorm), RunningNorm)
    tr = DeviceGAIL(demonstrations=demos, demo_batch_size=256, venv=venv, gen_algo=gen, reward_net=rn,
                    n_disc_updates_per_round=1, custom_logger=logger.configure("/tmp/ia_ppo_rc_record", format_strs=[]))
    tr._ppo_static["rc_gmax"] = case["gmax"]
    tr._ppo_static["rc_lean"] = case["rc_lean"]
    # Policy / value parameters from numpy's uniform stream (integer arithmetic only): torch's
    # orthogonal initialisation runs a host QR whose last bits follow the BLAS thread count, and
    # the recorded update has to come out the same under pytest and on another host. A non-zero
    # log_std also makes the entropy sum's order matter from the first minibatch on.
    g = np.random.default_rng(1000 + seed)
    with th.no_grad():
        for _, p in sorted(gen.policy.named_parameters()):
            scale = 1.0 / np.sqrt(p.shape[1]) if p.dim() == 2 else 0.1
            p.copy_(th.from_numpy(((2.0 * g.random(tuple(p.shape)) - 1.0) * scale).astype(np.float32)))
    return tr, gen


def _sha(t):
    a = np.ascontiguousarray(t.detach().cpu().numpy())
    return hashlib.sha256(str(a.dtype).encode() + b"|" + str(a.shape).encode() + b"|" + a.tobytes()).hexdigest()


def _digests(tensors):
    """name -> SHA-256; the parameter tensors fold into one digest (of their names and digests)."""
    each = {k: _sha(v) for k, v in tensors.items()}
    params = sorted(k for k in each if k.startswith("param/"))
    out = {k: v for k, v in each.items() if k not in params}
    out["params"] = hashlib.sha256("".join(f"{k}={each[k]};" for k in params).encode()).hexdigest()
    return out


def _written(tr, gen):
    """name -> tensor of everything the update writes."""
    out = {f"param/{n}": p for n, p in gen.policy.named_parameters()}
    out.update(exp_avg=tr.exp_avg, exp_avg_sq=tr.exp_avg_sq, adam_step=tr.adam_step)
    norm = tr.pol_norm
    if norm is not None:
        out.update(norm_mean=norm.running_mean, norm_var=norm.running_var, norm_count=norm.count)
    out["stats"] = tr.stats
    return out


def run_case(case):
    """Build the case's trainer, run one rollout and one update; returns (path, row, digests,
    names of the tensors the update changed)."""
    n_threads = th.get_num_threads()
    th.set_num_threads(1)  # (as the test suite's fixture: host-side initialisation is the same in both)
    try:
        tr, gen = build_trainer(case)
    finally:
        th.set_num_threads(n_threads)
    path = tr._C.engine_ppo_path(tr._ppo_static)
    row = tr._C.engine_ppo_row(tr._ppo_static)
    tr._rollout()
    before = {k: v.detach().clone() for k, v in _written(tr, gen).items()}
    tr._ppo_update()
    th.cuda.synchronize()
    tr.check_errors(blocking=True)
    after = _written(tr, gen)
    changed = sorted(k for k in after if not th.equal(after[k], before[k]))
    return path, row, _digests(after), changed


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--out", default=GOLDEN)
    a = ap.parse_args()
    rec = {}
    for case in CASES:
        path, row, dig, changed = run_case(case)
        if (path, row) != (case["path"], case["row"]):
            raise SystemExit(f"{case['name']}: runs {path} / {row}, the case table says {case['path']} / {case['row']}")
        if "exp_avg" not in changed or "stats" not in changed:
            raise SystemExit(f"{case['name']}: the update left exp_avg / stats untouched")
        rec[case["name"]] = dict(path=path, row=row, digests=dig)
        print(f"{case['name']}: {path} {row} ({len(dig)} tensors, {len(changed)} changed)", flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(rec, f, indent=1, sort_keys=True)
        f.write("\n")
    print(f"wrote {a.out}")


if __name__ == "__main__":
    main()
