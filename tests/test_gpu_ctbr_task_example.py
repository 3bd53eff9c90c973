"""examples/ctbr_task.py at 64 aviaries and 5 s: the hover task flown closed-loop through `VectorCTBRAviary.step()`, the controller's
own outer loop mapped into the [-1, 1] action space beside the idle action a = 0.  Finite figures, and the controller's mean episode
return above the idle action's: only the ordering is fixed in advance."""
import importlib.util
import math
import os

import pytest

from conftest import REPO

pytestmark = pytest.mark.gpu


def test_ctbr_task_example(gpu_device):
    spec = importlib.util.spec_from_file_location("example_ctbr_task", os.path.join(REPO, "examples", "ctbr_task.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    flown, idle = mod.run(drones=64, duration_sec=5.0, device=gpu_device)
    print(f"MEASURED ctbr_task at 64 aviaries, 5 s: controller (return, boxed, length) {flown}, idle {idle}")
    assert all(math.isfinite(v) for v in flown + idle)
    assert flown[2] > 0 and idle[2] > 0                    # episodes finished in both flights
    assert flown[0] > idle[0]
