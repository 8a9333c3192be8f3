"""The host plans of the register-chained PPO update (``engine_ppo_plan``: chosen kernel
instance, its template arguments, geometry, LDS, launch shape, workspace) over a fixed grid of
configurations, pinned against ``tests/golden/ppo_rc_plans.json``. Host-only: runs on CPU.

The golden file was written by the code that selected instances with hand-written shape
predicates, before the instance table (csrc/kernels/ppo_rc_instances.h) drove the choice; a
change to the table or the plan that moves any plan shows up here. After an INTENDED change of
plans, regenerate it with ``python tests/engine/test_ppo_plan_golden.py``.

Layout of the file, per environment override: ``named`` maps a case label to the plan dict of
each of its configurations (a rejected plan is the string ``"lds"``), compared key by key;
``sweep`` maps a block label to the SHA-256 of the JSON list of the block's 480 plans (the
950,400 plans of the sweep do not fit a committed file), so there every key of every plan is
compared through the digest and a failure names the blocks that moved.
"""

from __future__ import annotations

import hashlib
import itertools
import json
import os

GOLDEN = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "golden", "ppo_rc_plans.json")

# environment overrides every configuration is planned under
ENVS = {
    "default": {},
    "netsplit0": {"IMITATION_AMD_PPO_NETSPLIT": "0"},
    "bf3_0": {"IMITATION_AMD_PPO_BF3": "0"},
    "xchg2_0": {"IMITATION_AMD_PPO_XCHG2": "0"},
    "xchg2_1": {"IMITATION_AMD_PPO_XCHG2": "1"},
}
_KNOBS = ("IMITATION_AMD_PPO_NETSPLIT", "IMITATION_AMD_PPO_BF3", "IMITATION_AMD_PPO_XCHG2", "IMITATION_AMD_PPO_PLAN_DEBUG")

# (obs dim, action dim / count, discrete) of the envs the GPU tests build
_ENV = {"HalfCheetah": (17, 6, 0), "Walker2d": (17, 6, 0), "Hopper": (11, 3, 0), "CartPole": (4, 2, 1), "Pendulum": (3, 1, 0)}
TANH, RELU = 2, 1


def _cfg(D, A, discrete, pi_hidden, vf_hidden, act, batch, rows, rc_cus=256, rc_gmax=0, rc_cw=0, allow_rc=1, n_epochs=2):
    return dict(D=D, A=A, discrete=discrete, pi_dims=[D] + list(pi_hidden) + [A], vf_dims=[D] + list(vf_hidden) + [1],
                hidden_act=act, log_std_off=-1 if discrete else 0, batch=batch, rows=rows, n_epochs=n_epochs,
                rc_cus=rc_cus, rc_gmax=rc_gmax, rc_cw=rc_cw, allow_rc=allow_rc)


def _engine_case(env, allow_rc, batch, gmax, hidden=(32, 32), act=TANH, n_envs=None, n_steps=None):
    D, A, discrete = _ENV[env]
    n_envs = n_envs or (max(8, batch // 64) if batch > 64 else 4)  # (tests/engine/test_device_engine.py)
    n_steps = n_steps or (64 if batch > 256 else 32)
    return _cfg(D, A, discrete, hidden, hidden, act, batch, n_envs * n_steps, rc_gmax=gmax, allow_rc=allow_rc)


def named_cases():
    """label -> configurations: the shapes of test_ppo_kernel_matches_torch_reference and
    test_ppo_exchange_levels_are_bitwise_equal, and the cases of
    test_ppo_plan_caps_cooperating_groups_by_device_cus (all in test_device_engine.py)."""
    h64 = (64, 64)
    ref = [
        _engine_case("HalfCheetah", 1, 64, 0), _engine_case("HalfCheetah", 0, 64, 0),
        _engine_case("CartPole", 1, 64, 0), _engine_case("CartPole", 0, 64, 0),
        _engine_case("HalfCheetah", 1, 128, 0), _engine_case("HalfCheetah", 1, 128, 1),
        _engine_case("HalfCheetah", 1, 256, 2), _engine_case("CartPole", 1, 256, 0),
        _engine_case("Hopper", 1, 64, 0, h64), _engine_case("Hopper", 1, 256, 4, h64),
        _engine_case("Hopper", 1, 64, 0, h64, RELU), _engine_case("Hopper", 1, 512, 0, h64, RELU),
        _engine_case("Walker2d", 1, 128, 0, h64, RELU),
        _engine_case("Hopper", 1, 2048, 0, h64, RELU), _engine_case("Hopper", 1, 4096, 0, h64, RELU),
        _engine_case("HalfCheetah", 1, 64, 0, h64, RELU), _engine_case("CartPole", 1, 64, 0, h64),
        _engine_case("CartPole", 1, 128, 0, h64, RELU), _engine_case("HalfCheetah", 1, 64, 0, h64),
        _engine_case("HalfCheetah", 1, 128, 0, h64, RELU), _engine_case("Pendulum", 1, 64, 0, h64),
        _engine_case("Pendulum", 1, 32, 0),
    ]
    xchg = [
        _engine_case("HalfCheetah", 1, 512, 0, n_envs=16, n_steps=64),
        _engine_case("Hopper", 1, 2048, 0, h64, RELU, n_envs=32, n_steps=64),
        _engine_case("Hopper", 1, 4096, 0, h64, RELU, n_envs=64, n_steps=64),
    ]

    def caps(batch, cus, hidden=(32, 32), act=TANH, pi_hidden=None, D=17, A=6):
        return _cfg(D, A, 0, pi_hidden or hidden, hidden, act, batch, 4096, rc_cus=cus, n_epochs=0)

    cus = [
        caps(1024, 256), caps(1024, 16), caps(1024, 8), caps(64, 2), caps(64, 256, h64, TANH), caps(64, 256, h64, RELU),
        caps(64, 256, h64, pi_hidden=(64, 48)), caps(32, 256, D=3, A=1),
        caps(64, 256),  # (the test's last case leaves rc_cus to the device query: 256 without a device)
    ]
    return {"matches_torch_reference": ref, "exchange_levels": xchg, "caps_by_device_cus": cus}


_HIDDEN = {"32x32": ((32, 32), (32, 32)), "64x64": ((64, 64), (64, 64)), "64": ((64,), (64,)), "64x48": ((64, 48), (64, 48)),
           "32x32x32": ((32, 32, 32), (32, 32, 32)), "pi64x64_vf32x32": ((64, 64), (32, 32))}
_INNER = list(itertools.product((16, 32, 48, 64, 128, 512, 2048, 4096), (0, 16, 32, 64), (0, 2, 4), (2, 8, 16, 64, 256)))


def sweep_blocks():
    """label -> configurations: one block per (obs dim, hidden layout, activation, head), each
    over batch x rc_cw x rc_gmax x rc_cus."""
    for D, (hname, (pi_h, vf_h)), act, discrete in itertools.product(
            (1, 3, 4, 11, 16, 17, 20, 21, 32, 33, 64), _HIDDEN.items(), (1, 2, 3), (0, 1)):
        A = 2 if discrete else 6
        yield f"D{D}:{hname}:act{act}:{'cat' if discrete else 'gauss'}", [
            _cfg(D, A, discrete, pi_h, vf_h, act, batch, 8 * batch, rc_cus=cus, rc_gmax=gmax, rc_cw=cw)
            for batch, cw, gmax, cus in _INNER]


def _plan(C, cfg):
    p = C.engine_ppo_plan(cfg)
    return "lds" if p["path"] == "lds" else p


def compute(C):
    """The golden structure from the built extension. Sets and restores the planning knobs."""
    saved = {k: os.environ.pop(k, None) for k in _KNOBS}
    named = {env: {} for env in ENVS}
    sweep = {env: {} for env in ENVS}
    try:
        for part, out, cases in (("named", named, named_cases().items()), ("sweep", sweep, sweep_blocks())):
            for label, cfgs in cases:
                for env, knobs in ENVS.items():
                    os.environ.update(knobs)
                    plans = [_plan(C, cfg) for cfg in cfgs]
                    for k in knobs:
                        del os.environ[k]
                    if part == "sweep":  # 950,400 plans: the file keeps one digest per block
                        plans = hashlib.sha256(json.dumps(plans, sort_keys=True).encode()).hexdigest()
                    out[env][label] = plans
    finally:
        for k in _KNOBS:
            os.environ.pop(k, None)
        os.environ.update({k: v for k, v in saved.items() if v is not None})
    return {"named": named, "sweep": sweep}


def test_ppo_rc_plans_match_golden():
    from imitation_amd import _native

    got = compute(_native.load())
    with open(GOLDEN) as f:
        want = json.load(f)
    cases = named_cases()
    assert sum(len(c) for c in cases.values()) == 34 and len(got["sweep"]["default"]) == 11 * 6 * 3 * 2
    for env in ENVS:
        assert sorted(got["named"][env]) == sorted(want["named"][env])
        for label, cfgs in cases.items():
            g, w = got["named"][env][label], want["named"][env][label]
            assert len(g) == len(w) == len(cfgs)
            for cfg, gp, wp in zip(cfgs, g, w):
                assert gp == wp, f"{env} {label} {cfg}"  # every key of the plan dict
        bad = [b for b in want["sweep"][env] if got["sweep"][env].get(b) != want["sweep"][env][b]]
        assert not bad and len(got["sweep"][env]) == len(want["sweep"][env]), f"{env}: plans moved in blocks {bad}"


if __name__ == "__main__":
    import sys

    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
    from imitation_amd import _native

    with open(GOLDEN, "w") as f:
        json.dump(compute(_native.load()), f, separators=(",", ":"), sort_keys=True)
        f.write("\n")
    print("wrote", GOLDEN)
