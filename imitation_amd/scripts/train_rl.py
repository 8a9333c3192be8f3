"""Train a policy with RL, optionally on a learned reward (reference: src/imitation/scripts/train_rl.py).

Checkpoints: ``{log_dir}/policies/{step|final}/model.zip``, rollouts ``{log_dir}/rollouts/final.npz``
(an HF dataset directory, like the reference's ``data.serialize.save``).
"""

from __future__ import annotations

import logging
import pathlib
import warnings
from typing import Any, Mapping, Optional

import numpy as np

from imitation_amd.data import rollout, serialize as data_serialize, wrappers
from imitation_amd.envs.vec_env import VecNormalize
from imitation_amd.policies import serialize as policies_serialize
from imitation_amd.rewards.reward_wrapper import RewardVecEnvWrapper
from imitation_amd.rewards.serialize import load_reward
from imitation_amd.rl import callbacks
from imitation_amd.scripts.config.train_rl import train_rl_ex
from imitation_amd.scripts.config_engine import FileStorageObserver
from imitation_amd.scripts.ingredients import environment
from imitation_amd.scripts.ingredients import logging as logging_ingredient
from imitation_amd.scripts.ingredients import policy_evaluation, rl
from imitation_amd.utils import watchdog


def _make_device_trainer(engine: str, venv, normalize_reward: bool, normalize_kwargs: dict, reward_type: Optional[str],
                         agent_path: Optional[str]):
    """The device engine (:class:`imitation_amd.engine.rl.DevicePPO`: rollout, reward
    normalisation and PPO kernels) on the UNWRAPPED ``venv`` when ``engine`` is
    ``auto``/``device`` and the run is eligible, else None (the host loop). ``engine=device``
    fails loudly when it is not eligible; ``auto`` logs the reason."""
    if engine not in ("host", "auto", "device"):
        raise ValueError(f"engine must be 'host', 'auto' or 'device', got {engine!r}")
    if engine == "host":
        return None
    import torch as th

    from imitation_amd.engine import rl as device_rl

    if reward_type is not None:
        why = "training on a learned reward"
    elif agent_path is not None:
        why = "warm start from agent_path"
    elif not th.cuda.is_available():  # (before a PPO is built for nothing)
        why = "no GPU"
    else:
        algo = rl.make_rl_algo(venv)
        ok, why = device_rl.supports(venv, algo)
        if ok:
            try:
                trainer = device_rl.DevicePPO(algo, venv, normalize_reward=normalize_reward,
                                              normalize_kwargs=normalize_kwargs)
                logging.info("Using the device engine (DevicePPO)")
                return trainer
            except ValueError as e:  # e.g. nets too large for the persistent PPO kernel's LDS
                why = str(e)
    if engine == "device":
        raise ValueError(f"engine=device requested but unsupported: {why}")
    logging.info(f"Device engine not applicable ({why}); using the host loop")
    return None


@train_rl_ex.main
def train_rl(*, total_timesteps: int, normalize_reward: bool, normalize_kwargs: dict, reward_type: Optional[str],
             reward_path: Optional[str], load_reward_kwargs: Optional[Mapping[str, Any]], rollout_save_final: bool,
             rollout_save_n_timesteps: Optional[int], rollout_save_n_episodes: Optional[int], policy_save_interval: int,
             policy_save_final: bool, agent_path: Optional[str], engine: str, hub_install: bool, _run,
             _rnd: np.random.Generator) -> Mapping[str, float]:
    """Train an RL expert; returns ``rollout_stats`` of the final policy (+ ``engine_kind``)."""
    if hub_install and not policy_save_final:
        raise ValueError("hub_install installs the final policy: it needs policy_save_final")
    custom_logger, log_dir = logging_ingredient.setup_logging()
    rollout_dir = log_dir / "rollouts"
    policy_dir = log_dir / "policies"
    rollout_dir.mkdir(parents=True, exist_ok=True)
    policy_dir.mkdir(parents=True, exist_ok=True)
    with environment.make_venv(post_wrappers=[lambda env, idx: wrappers.RolloutInfoWrapper(env)]) as venv:
        callback_objs = []
        device_trainer = _make_device_trainer(engine, venv, normalize_reward, normalize_kwargs, reward_type, agent_path)
        if reward_type is not None:
            reward_fn = load_reward(reward_type, reward_path, venv, **(load_reward_kwargs or {}))
            venv = RewardVecEnvWrapper(venv, reward_fn)
            callback_objs.append(venv.make_log_callback())
            logging.info(f"Wrapped env in reward {reward_type} from {reward_path}.")
        if normalize_reward and device_trainer is None:
            venv = VecNormalize(venv, norm_obs=False, **normalize_kwargs)
            if reward_type == "RewardNet_normalized":
                warnings.warn("Applying normalization to already normalized reward function. Consider setting "
                              "normalize_reward as False", RuntimeWarning)
        if policy_save_interval > 0:
            callback_objs.append(callbacks.EveryNTimesteps(policy_save_interval,
                                                           policies_serialize.SavePolicyCallback(policy_dir)))
        callback = callbacks.CallbackList(callback_objs)
        if device_trainer is not None:
            algo = device_trainer.gen_algo
        else:
            algo = rl.make_rl_algo(venv) if agent_path is None else rl.load_rl_algo_from_path(agent_path=agent_path, venv=venv)
        algo.set_logger(custom_logger)
        with watchdog.cli_watchdog("train_rl") as wd:  # a rollout that never ends (stuck env / kernel) aborts the run
            callback.callbacks.append(watchdog.rl_beat_callback(wd))
            (device_trainer or algo).learn(total_timesteps, callback=callback)
        if rollout_save_final:
            sample_until = rollout.make_sample_until(rollout_save_n_timesteps, rollout_save_n_episodes)
            data_serialize.save(rollout_dir / "final.npz", rollout.rollout(algo, algo.get_env(), sample_until, rng=_rnd))
        if policy_save_final:
            policies_serialize.save_stable_model(policy_dir / "final", algo)
            if hub_install:  # where ``expert.policy_type=<algo>-huggingface`` looks first
                installed = policies_serialize.install_hub_model(policy_dir / "final" / "model.zip",
                                                                 type(algo).__name__.lower(),
                                                                 _run.config["environment"]["gym_id"])
                logging.info(f"Installed the expert as {installed}")
        stats = dict(policy_evaluation.eval_policy(algo, venv))
        stats["engine_kind"] = "device" if device_trainer is not None else "host"
        return stats


def main_console(argv=None):
    train_rl_ex.observers.append(FileStorageObserver(pathlib.Path.cwd() / "output" / "sacred" / "train_rl"))
    return train_rl_ex.run_commandline(argv)


if __name__ == "__main__":  # pragma: no cover
    main_console()
