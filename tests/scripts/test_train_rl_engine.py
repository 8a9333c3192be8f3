"""``train_rl``'s engine choice on a machine without a GPU, and the local hub install."""

import filecmp
import os

import pytest
import torch as th

from imitation_amd.policies import serialize

FAST = ["fast", "rl.fast", "environment.fast", "policy_evaluation.fast"]
TESTDATA = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "testdata")
CARTPOLE_EXPERT_ZIP = os.path.join(TESTDATA, "expert_models", "cartpole_0", "policies", "final", "model.zip")


@pytest.fixture
def no_gpu(monkeypatch):
    """A machine without a GPU (as the CPU test box is), wherever the test runs."""
    monkeypatch.setattr(th.cuda, "is_available", lambda: False)


@pytest.fixture(autouse=True)
def _chdir(tmp_path, monkeypatch):
    monkeypatch.chdir(tmp_path)


def _updates(tmp_path, **kw):
    return {"logging": {"log_root": str(tmp_path / "out")}, **kw}


def test_install_hub_model(tmp_path):
    hub = tmp_path / "hub"
    env = "seals/MadeUp-v7"
    dst = serialize.install_hub_model(CARTPOLE_EXPERT_ZIP, "ppo", env, hub=hub)
    assert dst == hub / "HumanCompatibleAI" / "ppo-seals-MadeUp-v7" / "model.zip"
    assert filecmp.cmp(dst, CARTPOLE_EXPERT_ZIP, shallow=False)
    other = tmp_path / "other.zip"
    other.write_bytes(b"replaced")
    assert serialize.install_hub_model(other, "ppo", env, hub=hub) == dst
    assert dst.read_bytes() == b"replaced"
    assert os.listdir(dst.parent) == ["model.zip"]  # no temporary file left behind


def test_installed_model_resolves(tmp_path, monkeypatch):
    monkeypatch.setenv("IMITATION_AMD_HUB", str(tmp_path / "hub"))
    with pytest.raises(FileNotFoundError):
        serialize.resolve_hub_model("ppo", "seals/MadeUp-v7")
    dst = serialize.install_hub_model(CARTPOLE_EXPERT_ZIP, "ppo", "seals/MadeUp-v7")  # hub=None: $IMITATION_AMD_HUB
    assert serialize.resolve_hub_model("ppo", "seals/MadeUp-v7") == dst


def test_engine_default_is_host():
    from imitation_amd.scripts.train_rl import train_rl_ex

    cfg = train_rl_ex.resolve_config([], {})
    assert cfg["engine"] == "host" and cfg["hub_install"] is False


def test_engine_bogus_raises(tmp_path):
    from imitation_amd.scripts.train_rl import train_rl_ex

    with pytest.raises(ValueError, match="engine must be"):
        train_rl_ex.run(named_configs=["cartpole", *FAST], config_updates=_updates(tmp_path, engine="bogus"))


def test_engine_device_without_gpu_raises(tmp_path, no_gpu):
    from imitation_amd.scripts.train_rl import train_rl_ex

    with pytest.raises(ValueError, match="engine=device requested but unsupported: no GPU"):
        train_rl_ex.run(named_configs=["cartpole", *FAST], config_updates=_updates(tmp_path, engine="device"))


def test_engine_auto_without_gpu_uses_host(tmp_path, no_gpu):
    from imitation_amd.scripts.train_rl import train_rl_ex

    run = train_rl_ex.run(named_configs=["cartpole", *FAST], config_updates=_updates(tmp_path, engine="auto"))
    assert run.status == "COMPLETED" and run.result["engine_kind"] == "host"
    assert "return_mean" in run.result


def test_device_ppo_refuses_without_gpu(cartpole_venv, no_gpu):
    from imitation_amd.engine import rl as device_rl
    from imitation_amd.rl.ppo import PPO

    algo = PPO("MlpPolicy", cartpole_venv, n_steps=16, batch_size=16, device="cpu")
    assert device_rl.supports(cartpole_venv, algo) == (False, "no GPU")
    with pytest.raises(ValueError, match="no GPU"):
        device_rl.DevicePPO(algo, cartpole_venv)
