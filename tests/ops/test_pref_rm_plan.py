"""The RunningNorm merge of the fused preference reward-model minibatch (``PrefRmPlan``:
csrc/kernels/pref_rm.hip, csrc/bind/pref.cpp) against float64 batch moments and Chan merge of
``imitation_amd.testing.disc_reference``; plans are built from plain tensors."""

import pytest
import torch as th

from imitation_amd.testing import disc_reference as dref

gpu = pytest.mark.gpu
F64 = th.float64
WARM_COUNT = 500

# (pairs, L, din): 2 rows; 30 rows, under one block; 154 rows = 2 x 64 + 26 (a ragged third block)
# with a second 64-column pass in the gather; exactly one block at the plan's 128 input columns;
# then the same row counts at 33 columns and at the 64 that reward_model.fused_check routes here.
SHAPES = [(1, 1, 1), (3, 5, 9), (7, 11, 65), (2, 16, 128), (7, 11, 33), (2, 16, 64)]


def _native():
    from imitation_amd import _native as nat

    return nat.load()


def _widths(din):
    """state | action | next state | done columns of a din-wide input (every part where it fits)."""
    if din < 4:
        return din, 0, 0, 0
    ds = (din - 1) // 2 - 1
    return ds, din - 1 - 2 * ds, ds, 1


def assert_norm(got, want):  # the bounds of assert_norm in test_disc_plan.py
    th.testing.assert_close(got["mean"].double(), want["mean"], rtol=1e-5, atol=1e-5)
    th.testing.assert_close(got["var"].double(), want["var"], rtol=1e-4, atol=1e-5)
    assert got["count"] == want["count"]


@gpu
@pytest.mark.parametrize("pairs,L,din", SHAPES)
def test_running_norm_merge_matches_fp64(pairs, L, din):
    """Two merging steps from a warm norm follow the float64 Chan merge of the gathered rows'
    two-pass moments in every column; a step with merge=False leaves the norm bitwise alone.
    Columns are drawn around the warm running mean at unit scale: the gather's sums are shifted
    by the running mean alone, which is only accurate there."""
    C = _native()
    dev = th.device("cuda")
    g = th.Generator().manual_seed(1000 * din + pairs)
    P, rows = pairs + 3, (pairs + 3) * 2 * L
    ds, da, dns, use_done = _widths(din)
    mean0 = 3.0 * th.randn(din, generator=g)
    var0 = 0.5 + th.rand(din, generator=g)
    data = mean0 + th.randn(rows, din, generator=g)  # dataset rows [pair * 2L + t]
    s_all, a_all, ns_all, d_all = (t.contiguous().to(dev) for t in data.split([ds, da, dns, use_done], 1))
    # one hidden layer of 32; at 128 columns that is 142912 bytes of LDS, over the plan's 128 KiB,
    # so the linear head alone (120384 bytes)
    dims = [din, 32, 1] if din < 128 else [din, 1]
    sizes = [n for i, o in zip(dims, dims[1:]) for n in (o * i, o)]  # flat order W0, b0, W1, b1
    flat = (0.1 * th.randn(sum(sizes), generator=g)).to(dev)
    parts = flat.split(sizes)
    W = [w.view(o, i) for w, i, o in zip(parts[0::2], dims, dims[1:])]
    b = list(parts[1::2])
    norm = dict(mean=mean0.to(dev), var=var0.to(dev), count=th.tensor(WARM_COUNT, dtype=th.int32, device=dev))
    z = lambda n: th.zeros(n, device=dev)  # noqa: E731
    plan = C.PrefRmPlan(dict(
        L=L, batch=pairs, capacity=pairs, ds=ds, da=da, dns=dns, use_done=use_done, s_all=s_all,
        a_all=a_all if da else None, ns_all=ns_all if dns else None, d_all=d_all.reshape(-1) if use_done else None,
        prefs_all=th.rand(P, generator=g).to(dev), gt_all=None, net=dict(W=W, b=b, hidden_act=1), rmean=norm["mean"],
        rvar=norm["var"], rcount=norm["count"], eps=1e-5, discount=0.99, threshold=50.0, noise=0.0, params=flat,
        exp_avg=z(flat.numel()), exp_avg_sq=z(flat.numel()), step=z(1), lr=1e-3, beta1=0.9, beta2=0.999, adam_eps=1e-8,
        weight_decay=0.0, decoupled=True))

    def gathered(idx):  # the minibatch's rows: pair idx[i] -> dataset rows idx[i] * 2L + [0, 2L)
        r = (idx[:, None] * 2 * L + th.arange(2 * L)[None, :]).reshape(-1)
        return data[r].to(F64)

    want = dref.norm_state(norm)
    for _ in range(2):
        idx = th.randperm(P, generator=g)[:pairs]
        plan.step(idx.to(dev), True)
        X = gathered(idx)
        want = dref.chan_merge(want, *dref.batch_moments(X), X.shape[0])
        assert_norm(dref.norm_state(norm), want)
    before = {k: v.clone() for k, v in norm.items()}
    plan.step(th.randperm(P, generator=g)[:pairs].to(dev), False)
    th.cuda.synchronize()
    for k, v in norm.items():
        assert th.equal(v.view(th.int32), before[k].view(th.int32)), k
