"""examples/avoid_task.py at 128 drones: the course of examples/avoid.py flown closed-loop through `VectorObstacleAviary.step()`, the
velocity command computed from the observation row alone.  The rule must end strictly fewer episodes in contact than the blind flight.

MEASURED on an MI355X (128 episodes of 8 s through 6 cylinders each), the share of episodes that ended collided:
    no rule 0.7266   clearance normal + forward ranges 0.0391"""
import importlib.util
import os

import pytest

from conftest import REPO

pytestmark = pytest.mark.gpu


def test_avoid_task_example(gpu_device):
    spec = importlib.util.spec_from_file_location("example_avoid_task", os.path.join(REPO, "examples", "avoid_task.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    blind, steered = mod.run(drones=128, device=gpu_device)
    print(f"MEASURED avoid_task at 128 drones: no rule {blind:.4f}, with the rule {steered:.4f}")
    assert 0.0 <= steered < blind <= 1.0
