"""``bc.engine`` on the command line (``train_imitation bc|dagger with ... bc.engine=...``)."""

import pytest

FAST = ["fast", "demonstrations.fast", "environment.fast", "policy_evaluation.fast"]


@pytest.fixture(autouse=True)
def _chdir(tmp_path, monkeypatch):
    monkeypatch.chdir(tmp_path)


def _updates(tmp_path, **kw):
    return {"logging": {"log_root": str(tmp_path / "out")}, **kw}


def test_config_default_is_the_host_engine():
    from imitation_amd.scripts.train_imitation import train_imitation_ex

    run = train_imitation_ex.run("print_config", named_configs=["cartpole", *FAST])
    assert run.config["bc"]["engine"] == "host"


def test_auto_runs_and_reports_the_engine_it_chose(tmp_path):
    """Without a GPU ``auto`` falls back to, and reports, the host engine."""
    import torch as th

    from imitation_amd.scripts.train_imitation import train_imitation_ex

    run = train_imitation_ex.run("bc", named_configs=["cartpole", *FAST], config_updates=_updates(tmp_path, bc={"engine": "auto"}))
    assert run.status == "COMPLETED" and "imit_stats" in run.result
    assert run.result["engine"] == ("device" if th.cuda.is_available() else "host")


@pytest.mark.gpu
@pytest.mark.parametrize("command", ["bc", "dagger"])
def test_device_engine_from_the_command_line(tmp_path, command):
    from imitation_amd.scripts.train_imitation import train_imitation_ex

    run = train_imitation_ex.run(command, named_configs=["cartpole", *FAST],
                                 config_updates=_updates(tmp_path, bc={"engine": "device"}))
    assert run.status == "COMPLETED" and "imit_stats" in run.result
    assert run.result["engine"] == "device"
