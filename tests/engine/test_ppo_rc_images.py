"""Row-major split-bf16 images of the register-chained PPO update (csrc/kernels/ppo_rc_kernel.h).

The activation / dZ images that feed the dW MFMAs hold, per 16-feature tile, a strip of
[batch row][16 features] bf16 values (hi = bf16(v), lo = bf16(v - hi)); a lane writes its four
consecutive features of a row with one 8-byte store and the dW operands come back through
``ds_read_b64_tr_b16``. ``engine_ppo_image_probe`` runs the kernel's own store and read helpers on
a given matrix and returns every operand fragment, so the lane map is checked element by element;
the update tests catch an image that is stale or not cleared between chunks, minibatches or calls.
"""

import importlib.util
import os

import numpy as np
import pytest
import torch as th

gpu = pytest.mark.gpu

_spec = importlib.util.spec_from_file_location(
    "_ia_test_device_engine_img", os.path.join(os.path.dirname(os.path.abspath(__file__)), "test_device_engine.py"))
_eng = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(_eng)
_setup = _eng._setup


def _bf16_bits(x):
    """float32 array -> bf16 bit patterns (uint16), round to nearest even."""
    b = np.ascontiguousarray(x, dtype=np.float32).view(np.uint32).astype(np.uint64)
    return ((b + 0x7FFF + ((b >> 16) & 1)) >> 16).astype(np.uint16)


def _bf16_val(bits):
    return (bits.astype(np.uint32) << 16).view(np.float32)


def _split(x):
    hi = _bf16_bits(x)
    lo = _bf16_bits(x.astype(np.float32) - _bf16_val(hi))
    return hi, lo


def _expected_fragments(x, rows_pad):
    """[2 (hi, lo)][tile][k-step][lane][8]: element j of lane (r16 = lane & 15, kk = lane >> 4) of
    k-step ks of feature tile t is batch row 32 ks + 8 kk + j of feature 16 t + r16 (rows past the
    matrix read 0)."""
    rows, feats = x.shape
    full = np.zeros((rows_pad, feats), np.float32)
    full[:rows] = x
    hi, lo = _split(full)
    lane = np.arange(64)
    r16, kk = lane & 15, lane >> 4
    out = np.zeros((2, feats // 16, rows_pad // 32, 64, 8), np.uint16)
    for t in range(feats // 16):
        for ks in range(rows_pad // 32):
            for j in range(8):
                r = 32 * ks + 8 * kk + j
                out[0, t, ks, :, j] = hi[r, 16 * t + r16]
                out[1, t, ks, :, j] = lo[r, 16 * t + r16]
    return out


@gpu
@pytest.mark.parametrize("mode", [0, 1], ids=["packed_store", "element_store"])
@pytest.mark.parametrize("rows,feats", [(64, 32), (32, 32), (16, 32), (64, 64)])
def test_image_probe_returns_every_operand_fragment(rows, feats, mode):
    """mode 0: the packed 8-byte store of hidden activations / dZ; mode 1: the per-element store
    of the layer-0 input image (its lane holds features 4 s + kk)."""
    from imitation_amd import _native

    C = _native.load()
    r = np.arange(rows, dtype=np.int64)[:, None]
    c = np.arange(feats, dtype=np.int64)[None, :]
    x = (r * 64 + c).astype(np.float32) + np.float32(2.0 ** -9) * (1 + (r + c) % 3).astype(np.float32)
    hi, lo = _split(x)
    assert hi.any() and (lo != 0).mean() > 0.5  # both halves carry data
    got = C.engine_ppo_image_probe(th.from_numpy(x).cuda(), mode)
    th.cuda.synchronize()
    rows_pad = max(rows, 32)
    want = _expected_fragments(x, rows_pad)
    got = got.cpu().numpy().view(np.uint16)
    assert got.shape == want.shape
    bad = np.argwhere(got != want)
    assert bad.size == 0, f"{len(bad)} fragment elements differ; first (half, tile, kstep, lane, j): {bad[0]}"


def _state(tr, gen):
    """Everything a PPO update writes: parameters, Adam state, normaliser state."""
    dst = list(gen.policy.parameters()) + [tr.exp_avg, tr.exp_avg_sq, tr.adam_step]
    norm = tr.pol_norm
    if norm is not None:
        dst += [norm.running_mean, norm.running_var, norm.count, tr.norm_count]
    return dst


def _update_from(tr, gen, s0, perm_round):
    dst = _state(tr, gen)
    with th.no_grad():
        for d, v in zip(dst, s0):
            d.copy_(v)
    tr._perm_round = perm_round
    tr._ppo_update()
    th.cuda.synchronize()
    return [t.detach().clone() for t in dst] + [tr.stats.detach().clone()]


@gpu
@pytest.mark.parametrize("env_id,batch,path", [
    ("seals/HalfCheetah-v1", 64, "rc:g1x1x64:kt2:ns"),
    ("Pendulum-v1", 32, "rc:g1x1x32:kt2"),  # run-time chunk width, 32-row images
])
def test_two_updates_from_one_state_are_bitwise_equal(env_id, batch, path):
    tr, venv, gen, rn = _setup(env_id=env_id, n_envs=4, n_steps=32, batch=batch, n_epochs=2)
    assert tr._C.engine_ppo_path(tr._ppo_static) == path
    tr._rollout()
    s0 = [t.detach().clone() for t in _state(tr, gen)]
    pr = tr._perm_round
    res = [_update_from(tr, gen, s0, pr) for _ in range(2)]
    tr.check_errors(blocking=True)
    assert any(not th.equal(a, b) for a, b in zip(res[0], s0))  # the update did something
    for i, (a, b) in enumerate(zip(res[0], res[1])):
        assert th.equal(a, b), f"tensor {i} differs between two updates from the same state"


@gpu
@pytest.mark.parametrize("gmax,path", [(1, "rc:g1x2x64:kt2:ns"), (0, "rc:g2x1x64:kt2:ns")])
def test_two_chunk_and_two_group_updates_run_clean(gmax, path):
    """Batch 128 as two chunks of one workgroup (the images are rewritten by the second chunk) and
    as two cooperating row groups (pre_rows writes the next minibatch's input image early)."""
    tr, venv, gen, rn = _setup(n_envs=8, n_steps=32, batch=128, n_epochs=2)
    tr._ppo_static["rc_gmax"] = gmax
    assert tr._C.engine_ppo_path(tr._ppo_static) == path
    tr._rollout()
    p0 = [p.detach().clone() for p in gen.policy.parameters()]
    tr._ppo_update()
    th.cuda.synchronize()
    tr.check_errors(blocking=True)
    p1 = list(gen.policy.parameters())
    assert all(bool(th.isfinite(p).all()) for p in p1)
    assert any(not th.equal(a, b) for a, b in zip(p0, p1))
