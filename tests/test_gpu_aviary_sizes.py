"""The launch shapes between the ones the other modules pin: aviaries of 16 to 99 drones, and single drones on narrow waves.

csrc/step_rollout.hip and csrc/gpd_common.inc choose their code from the shape of the call -- the lane -> drone map, the clone lanes of
a wave or workgroup that is not full, the wave-local LDS exchange of the downwash and of the MultiHover sums (`(D & 3) == 0`: groups of
four mates), the routing `drones_per_env <= 64` between gpd_rollout1_kernel and the compute-wave + store-wave kernel, the workgroup
packings (256 / D) D, and `GpdStepCfg.lanes_per_wave` = 16 / 32 with its own map, direct row stores and grid.  Here:
  * D in {16, 20, 32, 33, 48, 63, 64, 65, 85, 86, 99}: one step against the float64 oracle (bound 5e-5, the large-aviary test's: these
    downwash sums are shorter than its 255 terms), a rollout against K single steps bit for bit (both rollout kernels), the fused
    action ring at 64 and 33 drones;
  * lanes_per_wave 16 and 32 against a twin at 64, bit for bit.
Scenes are the tall column of tests/helpers/aviary_sizes.py; every batch is the smallest that gives two workgroups and a ragged last
one (`ragged_envs`), or one aviary."""
import os
import sys
import zlib

import numpy as np
import pytest
import torch

from conftest import REPO, urdf
from oracle.batched_oracle import BatchedAviary
from test_gpu_parity import _actions, _core, _oracle_kin, _random_scene, _sync_from_oracle
from test_gpu_rollout import test_rollout_with_lazy_history_pushes_the_ring_inside_the_kernel as _lazy_history_case

sys.path.insert(0, os.path.join(REPO, "tests", "helpers"))
from aviary_sizes import STATE, column_top, ragged_envs, rollout_equals_steps, tall_column  # noqa: E402

pytestmark = pytest.mark.gpu

SIZES = [16, 20, 32, 33, 48, 63, 64, 65, 85, 86, 99]


def _seed(*key):
    return zlib.crc32(repr(key).encode())


# ---- 1a: one step against the float64 oracle ------------------------------------------------------------------------------------
ONE_STEP = [(D, 7, "rpm") for D in SIZES] + [(16, 31, "rpm"), (33, 31, "rpm"), (64, 4, "rpm"), (65, 4, "rpm"), (16, 7, "pid"), (33, 7, "pid")]


@pytest.mark.parametrize("D,flags,act", ONE_STEP)
def test_one_step_of_every_aviary_size_against_the_oracle(gpu_device, D, flags, act):
    """Three control steps of two sub-steps, MultiHover, from the oracle's state rounded to fp32: kinematic rows within 5e-5 of each
    row's scale, reward, `truncated` and the step counters -- as test_largest_aviaries_one_workgroup_per_aviary compares them.  The
    step kernel exchanges wave-locally at 16, 32 and 64 drones (groups of four mates) and through workgroup barriers at every other
    size, in workgroups of 231 (D = 33), 195 (65), 255 (85), 172 (86) ... lanes, the last one ragged."""
    rng = np.random.default_rng(_seed("one step", D, flags, act))
    E, S = ragged_envs(D), 2
    xyz, rpy = tall_column(rng, E, D)
    b = BatchedAviary(urdf("cf2x"), "cf2x", num_envs=E, num_drones=D, initial_xyzs=xyz, initial_rpys=rpy, physics_flags=flags,
                      pyb_freq=240, ctrl_freq=240 // S, act=act, task="multihover", pid_urdf_path=urdf("cf2x"))
    core = _core("cf2x", E, D, flags, S, act, "multihover", xyz, rpy, gpu_device, target=b.TARGET_POS)
    _sync_from_oracle(core, b)
    worst = 0.0
    for k in range(3):
        if act == "pid":
            a = (xyz + np.array([0, 0, 0.2]) + 0.05 * rng.uniform(-1, 1, size=(E, D, 3))).astype(np.float32)
        else:
            a = (0.05 * rng.uniform(-1, 1, size=(E, D, 4))).astype(np.float32)
        obs, rew, term, trunc, _ = b.step(a.astype(np.float64))
        core.step(torch.as_tensor(a, device=gpu_device))
        kin = core.kin[:, :E * D].cpu().numpy().astype(np.float64)
        ref = _oracle_kin(b)
        err = np.abs(kin - ref) / np.maximum(np.abs(ref).max(axis=1, keepdims=True), 1.0)
        worst = max(worst, float(err.max()))
        print(f"one step, D = {D}, flags {flags}, {act}, E = {E}, step {k}: max scaled |kin - oracle| = {err.max():.3e}, "
              f"max |reward - oracle| = {np.abs(core.reward.cpu().numpy() - rew).max():.3e}")
        assert err.max() < 5e-5, (k, err.max(axis=1))
        # the reward is a sum over the aviary's drones of values <= 2: compare relative to its size
        np.testing.assert_allclose(core.reward.cpu().numpy(), rew, rtol=2e-5, atol=1e-4)
        np.testing.assert_array_equal(core.truncated.cpu().numpy().astype(bool), trunc)
        np.testing.assert_array_equal(core.step_counter.cpu().numpy(), b.step_counter)
    print(f"one step, D = {D}, flags {flags}, {act}: worst of three steps {worst:.3e}")


# ---- 1b: one rollout of K steps is K single steps, bit for bit -------------------------------------------------------------------
BITWISE = [(D, ragged_envs(D), "rpm") for D in SIZES] + [(32, ragged_envs(32), "pid"), (33, ragged_envs(33), "pid"), (33, 1, "rpm"), (65, 1, "rpm")]


@pytest.mark.parametrize("keep_term", [False, True])
@pytest.mark.parametrize("S", [1, 2])
@pytest.mark.parametrize("D,E,act", BITWISE)
def test_rollout_of_every_aviary_size_is_bitwise_k_steps(gpu_device, D, E, act, S, keep_term):
    """K = 12 steps with every force term, auto-reset on.  Without terminal observations aviaries of up to 64 drones run
    gpd_rollout1_kernel (whole aviaries per wave: 33 drones leave 31 pad lanes per wave, clones of the wave's first aviary; the
    exchange is wave-local at every size), with them and above 64 drones the compute-wave + store-wave kernel (workgroups of
    (256 / D) D lanes, aviaries that span waves); the K single steps run gpd_step_kernel.  z_bound is above the column and an episode
    lasts 10 physics steps, so aviaries end by time, and -- a drone in every third aviary turns at 20 rad/s -- by tilt before that:
    some (aviary, step) pairs end inside the window, not all."""
    rng = np.random.default_rng(_seed("bitwise", D, E, act, S))
    K, flags = 12, 7
    xyz, rpy = tall_column(rng, E, D)
    mk = lambda: _core("cf2x", E, D, flags, S, act, "multihover", xyz, rpy, gpu_device, auto_reset=True,  # noqa: E731
                       target=xyz + np.array([0, 0, 0.3]), keep_term=keep_term)
    a, b = mk(), mk()
    for c in (a, b):
        c._cfg.z_bound = column_top(D)
        c._cfg.trunc_counter = 10
    kin = a.kin.clone()
    kin[7:13] = torch.as_tensor(rng.uniform(-0.5, 0.5, size=(6, a.ld)), dtype=torch.float32, device=gpu_device)
    spinning = [e * D + (7 * e) % D for e in range(0, E, 3)]
    kin[10, spinning] = 20.0
    a.set_state(kin=kin[:, :a.N]); b.set_state(kin=kin[:, :b.N])
    if act == "pid":
        acts = xyz + np.array([0, 0, 0.2]) + 0.05 * rng.uniform(-1, 1, size=(K, E, D, 3))
    else:
        acts = rng.uniform(-1, 1, size=(K, E, D, 4))
    te_s, tr_s = rollout_equals_steps(a, b, torch.as_tensor(acts.astype(np.float32), device=gpu_device), keep_term)
    done = te_s | tr_s
    assert done.any() and not done.all(), "some (aviary, step) pairs must end inside the window, not all"
    if E >= 4 and act == "rpm":     # by tilt (the aviaries with a spinning drone, first) and by time (the others, together)
        first = done.float().argmax(dim=0).cpu().numpy()
        assert (first[::3] < first[1]).all() and (first[1::3] == first[1]).all(), first


# ---- 1c: the action ring pushed inside the rollout kernel, with pad lanes -----------------------------------------------------------
@pytest.mark.parametrize("D,E", [(64, ragged_envs(64)), (33, ragged_envs(33))])
def test_fused_history_ring_with_pad_lanes(gpu_device, D, E):
    """`gpd_rollout_history` (the RING instantiations of gpd_rollout1_kernel) at 64 drones -- full waves, a ragged last workgroup whose
    spare waves are clones -- and at 33: 31 pad lanes per wave push their original's action into their original's slot.  The
    comparison is test_rollout_with_lazy_history_pushes_the_ring_inside_the_kernel's, on the tall column with every force term."""
    rng = np.random.default_rng(_seed("ring", D))
    xyz, rpy = tall_column(rng, E, D)
    _lazy_history_case(gpu_device, "rpm", D, 48, E, 12, True, scene=(dict(initial_xyzs=xyz, initial_rpys=rpy, physics=7, track_rpm=True), column_top(D)))


# ---- 2: single drones on narrow waves ------------------------------------------------------------------------------------------------
def _twins(dev, rng, E, act, flags, S, keep_term=True, history=True):
    """two identical cores of E single-drone aviaries with short episodes, auto-reset, terminal observations and an action ring"""
    xyz, rpy = _random_scene(rng, E, 1)
    if flags & 8:          # a third of the aviaries start within centimetres of the ground plane
        xyz[::3, :, 2] = rng.uniform(0.0, 0.04, size=xyz[::3, :, 2].shape)
    mk = lambda: _core("cf2x", E, 1, flags, S, act, "hover", xyz, rpy, dev, auto_reset=True, target=xyz + np.array([0, 0, 0.3]),  # noqa: E731
                       keep_term=keep_term)
    n, w = mk(), mk()
    kin = n.kin.clone()
    kin[7:13] = torch.as_tensor(rng.uniform(-0.5, 0.5, size=(6, n.ld)), dtype=torch.float32, device=dev)
    for c in (n, w):
        c._cfg.trunc_counter = 10 * S          # (ten control steps: three episodes in 30 steps, plus the out-of-bounds ones)
        c.set_state(kin=kin[:, :c.N])
        if history:
            c.enable_history(15)
    return n, w


def _same_state(n, w):
    for name in STATE + ("term_obs12", "act_ring", "ring_pos"):
        x, y = getattr(n, name), getattr(w, name)
        assert (x is None) == (y is None), name
        if x is not None:
            assert torch.equal(x, y), name


def _step_both(n, w, acts, E, narrow_call=None):
    """every block of `acts` through both cores: every output of every step with equal bits, then the state; returns truncated [K, E]"""
    tr_s = []
    for k in range(acts.shape[0]):
        on = [t.clone() for t in (narrow_call(k) if narrow_call else n.step(acts[k]))]
        ow = [t.clone() for t in w.step(acts[k])]
        for i, (x, y) in enumerate(zip(on, ow)):
            assert torch.equal(x.reshape(y.shape), y), (k, i)
        if n.term_obs12 is not None:
            assert torch.equal(n.term_obs12, w.term_obs12), k
        tr_s.append(ow[3])
    _same_state(n, w)
    return torch.stack(tr_s)


NARROW = [(lanes, E, act, flags) for lanes in (16, 32) for E in (1, 5, 17, 70, 1000) for act in ("rpm", "one_d_rpm", "pid") for flags in (0, 7, 24)]


@pytest.mark.parametrize("lanes,E,act,flags", NARROW)
def test_narrow_waves_are_bitwise_the_full_wave(gpu_device, lanes, E, act, flags):
    """`GpdStepCfg.lanes_per_wave` = 16 / 32: gpd_step_kernel then maps (workgroup, wave, lane) to a drone differently (4 x 16 or 4 x 32
    drones per workgroup, the upper lanes of every wave idle), stores its observation rows directly instead of through the LDS transpose
    and runs on a larger grid.  30 steps with auto-reset and episodes of ten steps: every output of every step, the terminal
    observations, the state, the action ring and its positions equal a twin at 64 lanes, bit for bit.  One sub-step per step and eight
    alternate over the cases (`S`)."""
    S = (1, 8)[(NARROW.index((lanes, E, act, flags)) // 3) % 2]
    rng = np.random.default_rng(_seed("narrow", E, act, flags, S))
    n, w = _twins(gpu_device, rng, E, act, flags, S)
    n._cfg.lanes_per_wave = lanes
    assert w._cfg.lanes_per_wave == 64
    acts = torch.as_tensor(_actions(rng, act, (30, E, 1), n.P.HOVER_RPM).astype(np.float32), device=gpu_device)
    tr = _step_both(n, w, acts, E)
    assert tr.any() and not tr.all(), "episodes must end inside the 30 steps, and not at every step"
    assert int(n.ring_pos[0]) == 0 and n.act_ring.abs().sum() > 0            # (30 pushes into a ring of 15)


@pytest.mark.parametrize("lanes", [16, 32])
def test_lanes_per_wave_from_the_environment(gpu_device, monkeypatch, lanes):
    """GPD_LANES_PER_WAVE is read when a core is built (`engine.lanes_per_wave`) and reaches the kernel: same bits as the twin at 64."""
    rng = np.random.default_rng(_seed("narrow env", lanes))
    E, S = 70, 1
    xyz, rpy = _random_scene(rng, E, 1)
    mk = lambda: _core("cf2x", E, 1, 7, S, "rpm", "hover", xyz, rpy, gpu_device, auto_reset=True, target=xyz + np.array([0, 0, 0.3]),  # noqa: E731
                       keep_term=True)
    monkeypatch.delenv("GPD_LANES_PER_WAVE", raising=False)
    w = mk()
    monkeypatch.setenv("GPD_LANES_PER_WAVE", str(lanes))
    n = mk()
    monkeypatch.delenv("GPD_LANES_PER_WAVE")
    assert n._cfg.lanes_per_wave == lanes and w._cfg.lanes_per_wave == 64
    for c in (n, w):
        c._cfg.trunc_counter = 10
    acts = torch.as_tensor(_actions(rng, "rpm", (30, E, 1), n.P.HOVER_RPM).astype(np.float32), device=gpu_device)
    tr = _step_both(n, w, acts, E)
    assert tr.any() and not tr.all()


@pytest.mark.parametrize("lanes,E", [(16, 70), (32, 1000)])
def test_one_step_rollout_on_narrow_waves(gpu_device, lanes, E):
    """A rollout of one step is routed to gpd_step_kernel, `lanes_per_wave` and its grid included: 30 of them equal the twin's 30
    single steps at 64 lanes (a rollout does not push into the action ring: none here)."""
    rng = np.random.default_rng(_seed("narrow rollout", lanes, E))
    n, w = _twins(gpu_device, rng, E, "rpm", 7, 1, keep_term=False, history=False)
    n._cfg.lanes_per_wave = lanes
    acts = torch.as_tensor(_actions(rng, "rpm", (30, E, 1), n.P.HOVER_RPM).astype(np.float32), device=gpu_device)
    tr = _step_both(n, w, acts, E, narrow_call=lambda k: n.rollout(acts[k:k + 1]))
    assert tr.any() and not tr.all()
