"""Import layering of the device engines (CPU): the generator core stands below every trainer.

``engine.generator`` must load none of the trainers built on it, a plain ``train_rl`` engine
must not load the adversarial engines, and the preference-comparison engine must not either.
Each check runs in a fresh interpreter, so nothing this test session imported counts."""

import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
_ADVERSARIAL = ("imitation_amd.engine.adversarial", "imitation_amd.engine.gail", "imitation_amd.engine.airl")

CASES = {
    "imitation_amd.engine.generator": _ADVERSARIAL + ("imitation_amd.engine.preference",
                                                      "imitation_amd.algorithms.adversarial.common",
                                                      "imitation_amd.algorithms.preference_comparisons"),
    "imitation_amd.engine.rl": _ADVERSARIAL,
    "imitation_amd.engine.preference": _ADVERSARIAL,
}


@pytest.mark.parametrize("module", sorted(CASES))
def test_engine_module_does_not_load_the_trainers_above_it(module):
    code = (f"import sys, {module}\n"
            f"print(','.join(m for m in {CASES[module]!r} if m in sys.modules))")
    out = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=300, cwd=ROOT)
    assert out.returncode == 0, out.stderr
    assert out.stdout.strip() == "", f"importing {module} also loaded {out.stdout.strip()}"
