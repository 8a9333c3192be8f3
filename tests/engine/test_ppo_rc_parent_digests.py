"""The register-chained PPO update against digests recorded before a kernel change.

tests/golden/ppo_rc_update_digests.json holds, per case of tools/ppo_rc_record.py, the SHA-256
of everything one update leaves behind (parameters, Adam moments and step, normaliser state, the
five PPO statistics), recorded on an MI355X with the build of the commit before the per-minibatch
code of csrc/kernels/ppo_rc_kernel.h was last reordered. A change that only moves work between
the barriers must reproduce every one of them bit for bit.
"""

import importlib.util
import json
import os

import pytest

gpu = pytest.mark.gpu

_ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
_spec = importlib.util.spec_from_file_location("_ia_ppo_rc_record", os.path.join(_ROOT, "tools", "ppo_rc_record.py"))
_rec = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(_rec)

with open(_rec.GOLDEN) as _f:
    _GOLD = json.load(_f)


def test_every_case_has_a_recorded_digest():
    assert sorted(_GOLD) == sorted(c["name"] for c in _rec.CASES)
    for c in _rec.CASES:
        g = _GOLD[c["name"]]
        assert (g["path"], g["row"]) == (c["path"], c["row"])
        assert {"exp_avg", "exp_avg_sq", "adam_step", "stats"} <= set(g["digests"])
        assert ("norm_mean" in g["digests"]) == c["normalize"]


@gpu
@pytest.mark.parametrize("case", _rec.CASES, ids=[c["name"] for c in _rec.CASES])
def test_update_reproduces_the_recorded_digests(case):
    gold = _GOLD[case["name"]]
    path, row, dig, changed = _rec.run_case(case)
    # the case still runs the kernel instance it was recorded on
    assert (path, row) == (case["path"], case["row"]) == (gold["path"], gold["row"])
    assert "exp_avg" in changed and "stats" in changed  # the update did something
    assert sorted(dig) == sorted(gold["digests"])
    diff = [k for k in sorted(dig) if dig[k] != gold["digests"][k]]
    assert not diff, f"{case['name']}: {diff} differ from the recorded update"
