"""Lean single-row-group rows of the register-chained PPO update (csrc/kernels/ppo_rc_instances.h).

A lean row is its full twin with the partial exchange and the cycle counters compiled out; the
plan takes it for one row group (G == 1) without a ``prof`` tensor unless ``rc_lean = 0``. Both
rows run the same arithmetic in the same order, so their updates must be bitwise equal.
"""

import importlib.util
import os

import pytest
import torch as th

gpu = pytest.mark.gpu

_spec = importlib.util.spec_from_file_location(
    "_ia_test_device_engine", os.path.join(os.path.dirname(os.path.abspath(__file__)), "test_device_engine.py"))
_eng = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(_eng)
_setup, _plan_dict = _eng._setup, _eng._plan_dict


def _state(tr, gen):
    """Everything a PPO update writes: parameters, Adam state, normaliser state, PPO stats."""
    dst = list(gen.policy.parameters()) + [tr.exp_avg, tr.exp_avg_sq, tr.adam_step]
    norm = tr.pol_norm
    if norm is not None:
        dst += [norm.running_mean, norm.running_var, norm.count, tr.norm_count]
    return dst


def _update_from(tr, gen, s0, perm_round, rc_lean):
    dst = _state(tr, gen)
    with th.no_grad():
        for d, v in zip(dst, s0):
            d.copy_(v)
    tr._perm_round = perm_round
    tr._ppo_static["rc_lean"] = rc_lean
    tr._ppo_update()
    th.cuda.synchronize()
    return [t.detach().clone() for t in dst] + [tr.stats.detach().clone()]


@gpu
@pytest.mark.parametrize("env_id,batch,n_envs,gmax,net_arch,path,rows", [
    # 2 minibatches per epoch
    ("seals/HalfCheetah-v1", 64, 4, 0, None, "rc:g1x1x64:kt2:ns", ("ns_cheetah32_lean", "ns_cheetah32")),
    ("seals/CartPole-v0", 64, 4, 0, None, "rc:g1x1x64:kt2:ns", ("ns_cartpole32_lean", "ns_cartpole32")),
    # two chunks per minibatch: the prefetched operands are reused across the chunks
    ("seals/HalfCheetah-v1", 128, 8, 1, None, "rc:g1x2x64:kt2:ns", ("ns_cheetah32_lean", "ns_cheetah32")),
    # the lean 64-wide row
    ("seals/Hopper-v1", 64, 4, 0, dict(pi=[64, 64], vf=[64, 64]), "rc:g1x1x64:kt4:ns", ("ns_hopper64r_lean", "ns_hopper64r")),
])
def test_lean_row_is_bitwise_the_full_row(env_id, batch, n_envs, gmax, net_arch, path, rows):
    act = th.nn.ReLU if net_arch is not None else None
    tr, venv, gen, rn = _setup(env_id=env_id, n_envs=n_envs, n_steps=32, batch=batch, n_epochs=2, net_arch=net_arch,
                               activation=act)
    tr._ppo_static["rc_gmax"] = gmax
    got = []
    for lean in (1, 0):
        tr._ppo_static["rc_lean"] = lean
        assert tr._C.engine_ppo_path(tr._ppo_static) == path
        got.append(tr._C.engine_ppo_row(tr._ppo_static))
    assert tuple(got) == rows  # the two runs below really take different rows
    tr._rollout()
    s0 = [t.detach().clone() for t in _state(tr, gen)]
    pr = tr._perm_round
    res = [_update_from(tr, gen, s0, pr, lean) for lean in (1, 0)]
    tr.check_errors(blocking=True)
    assert any(not th.equal(a, b) for a, b in zip(res[0], s0))  # the update did something
    for i, (a, b) in enumerate(zip(res[0], res[1])):
        assert th.equal(a, b), f"tensor {i} differs between the lean and the full row"


@gpu
def test_row_selection_keeps_full_rows_for_groups_and_counters():
    # G > 1 (batch 128 at the default rc_gmax: two row groups): the full row, whatever rc_lean says
    tr, venv, gen, rn = _setup(n_envs=8, n_steps=32, batch=128, n_epochs=2)
    for lean in (0, 1):
        tr._ppo_static["rc_lean"] = lean
        assert tr._C.engine_ppo_path(tr._ppo_static) == "rc:g2x1x64:kt2:ns"
        assert tr._C.engine_ppo_row(tr._ppo_static) == "ns_cheetah32"
    # G == 1 with cycle counters: the full row (the counters live there)
    tr, venv, gen, rn = _setup(n_envs=4, n_steps=32, batch=64, n_epochs=2)
    tr._ppo_static["rc_lean"] = 1
    assert tr._C.engine_ppo_row(tr._ppo_static) == "ns_cheetah32_lean"
    tr._ppo_static["prof"] = th.zeros(20, dtype=th.int64, device="cuda")
    assert tr._C.engine_ppo_path(tr._ppo_static) == "rc:g1x1x64:kt2:ns"
    assert tr._C.engine_ppo_row(tr._ppo_static) == "ns_cheetah32"
    tr._rollout()
    tr._ppo_update()
    th.cuda.synchronize()
    tr.check_errors(blocking=True)
    assert int(tr._ppo_static["prof"][0]) > 0  # the full row ran: it filled the counters


def test_plan_binding_is_host_only_and_paths_do_not_move():
    """engine_ppo_path gives the strings of test_ppo_plan_caps_cooperating_groups_by_device_cus
    (test_device_engine.py) with rc_lean 0 and 1; engine_ppo_row names the launched row. CPU."""
    from imitation_amd import _native

    C = _native.load()
    d48 = _plan_dict(64, 4096, 256, width=64)
    d48["pi_dims"] = [17, 64, 48, 6]
    d32 = _plan_dict(32, 4096, 256)
    d32["D"], d32["pi_dims"], d32["vf_dims"] = 3, [3, 32, 32, 1], [3, 32, 32, 1]
    cases = [
        (_plan_dict(1024, 4096, 256), "rc:g16x1x64:kt2:ns", "ns_cheetah32", "ns_cheetah32"),
        (_plan_dict(1024, 4096, 16), "rc:g4x4x64:kt2:ns", "ns_cheetah32", "ns_cheetah32"),
        (_plan_dict(1024, 4096, 8), "rc:g2x8x64:kt2:ns", "ns_cheetah32", "ns_cheetah32"),
        (_plan_dict(64, 4096, 2), "lds", "lds", "lds"),
        (_plan_dict(64, 4096, 256, width=64, act=2), "rc:g1x1x64:kt4:ns", "ns_64_d32_tanh_gauss", "ns_64_d32_tanh_gauss"),
        (_plan_dict(64, 4096, 256, width=64, act=1), "rc:g1x1x64:kt4:ns", "ns_walker64r_lean", "ns_walker64r"),
        (d48, "lds", "lds", "lds"),
        (d32, "rc:g1x1x32:kt2", "narrow32", "narrow32"),
        (_plan_dict(64, 4096, 256), "rc:g1x1x64:kt2:ns", "ns_cheetah32_lean", "ns_cheetah32"),
    ]
    for d, path, lean_row, full_row in cases:
        assert C.engine_ppo_row(d) == lean_row  # rc_lean defaults to 1
        for lean, row in ((1, lean_row), (0, full_row)):
            d = dict(d, rc_lean=lean)
            assert C.engine_ppo_path(d) == path
            assert C.engine_ppo_row(d) == row
            plan = C.engine_ppo_plan(d)
            if path != "lds":  # the plan reports the shape's full row whichever twin launches
                assert plan["instance"] == full_row and plan["path"] == path
    d = _plan_dict(64, 4096, 0)  # the device query is the default (no device: the MI355X count)
    for lean in (0, 1):
        assert C.engine_ppo_path(dict(d, rc_lean=lean)).startswith("rc:g1x1x64")
    # a prof entry keeps the full row; planning never touches the tensor's memory
    d = dict(_plan_dict(64, 4096, 256), prof=th.zeros(20, dtype=th.int64))
    assert C.engine_ppo_row(d) == "ns_cheetah32"
