"""`gpd_rollout` (K env steps per launch, state in registers) against K calls of `gpd_step` -- bitwise --
and against the float64 oracle stepped K times."""
import os
import sys
import zlib

import numpy as np
import pytest
import torch

from conftest import REPO, urdf
from oracle.batched_oracle import BatchedAviary
from test_gpu_parity import _actions, _core, _oracle_kin, _random_scene, _sync_from_oracle

sys.path.insert(0, os.path.join(REPO, "tests", "helpers"))
from aviary_sizes import rollout_equals_steps  # noqa: E402

pytestmark = pytest.mark.gpu

CASES = [  # act, flags, D, S, model
    ("rpm", 0, 1, 1, "cf2x"), ("rpm", 0, 1, 8, "cf2p"), ("one_d_rpm", 7, 1, 2, "racer"), ("pid", 0, 1, 1, "cf2x"),
    ("pid", 7, 3, 2, "cf2x"), ("vel", 2, 2, 4, "cf2p"), ("one_d_pid", 5, 8, 1, "cf2x"), ("raw_rpm", 7, 5, 2, "racer"),
    ("rpm", 4, 2, 8, "cf2x"),
    ("rpm", 15, 1, 2, "cf2x"), ("one_d_rpm", 9, 4, 8, "cf2p"),      # the ground plane (GPD_PHYS_GROUND = 8) in both rollout kernels
    ("rpm", 24, 1, 1, "cf2x"), ("pid", 31, 3, 2, "cf2x"),           # Bullet's default damping (GPD_PHYS_DAMP = 16), what Physics.PYB resolves to
]


def _pair(act, flags, D, S, model, dev, E, rng, auto_reset=True, keep_term=True):
    task = "none" if act == "raw_rpm" else ("hover" if D == 1 else "multihover")
    xyz, rpy = _random_scene(rng, E, D)
    if flags & 8:          # a third of the aviaries start on / within centimetres of the ground plane
        xyz[::3, :, 2] = rng.uniform(0.0, 0.04, size=xyz[::3, :, 2].shape) + (0.3 * np.arange(D) if D > 1 else 0.0)
    tgt = None if task == "none" else xyz + np.array([0, 0, 0.3])
    mk = lambda: _core(model, E, D, flags, S, act, task, xyz, rpy, dev, auto_reset=auto_reset, target=tgt,  # noqa: E731
                       keep_term=keep_term)
    return mk(), mk()


RAGGED = [  # act, flags, D, S, model, E, K: ragged last workgroups, whole-aviary packing (D = 3: 255 lanes), tiny and
            # large batches (> 131 072 drones switches the LDS ring from 4 to 2 slots), K not a multiple of 3
    ("rpm", 0, 1, 1, "cf2x", 1000, 7), ("pid", 0, 1, 2, "cf2x", 257, 5), ("rpm", 4, 3, 1, "cf2x", 100, 8),
    ("one_d_rpm", 0, 1, 1, "cf2x", 5, 4), ("raw_rpm", 2, 7, 2, "cf2p", 37, 6), ("rpm", 0, 1, 1, "cf2x", 140001, 10),
    ("vel", 7, 2, 1, "cf2x", 70001, 5), ("rpm", 0, 1, 1, "cf2x", 1, 2),
    ("rpm", 2, 1, 3, "cf2x", 300, 7), ("pid", 7, 1, 5, "cf2p", 200, 4),       # odd sub-step counts
    # more workgroups than the chip holds at once (256 CUs x 8) AND a ragged tail: the clone lanes of the last workgroup
    # start long after workgroup 0 has finished and rewritten its state (round-1 advisor finding)
    ("rpm", 0, 1, 1, "cf2x", 1200001, 6), ("rpm", 4, 2, 1, "cf2x", 600001, 5),
    # K >= 48 at up to 2^17 plain RPM drones, one sub-step: the ordinary-store instantiation of gpd_rollout1_kernel (`plain_obs`, what a
    # default 64-step launch runs) -- a ragged batch (clone lanes), five drones, one drone, K = 0, 1, 2 mod 3 of the three-step loop --
    # and K = 47, the last one on the non-temporal side
    ("rpm", 0, 1, 1, "cf2x", 1000, 48), ("rpm", 0, 1, 1, "cf2x", 5, 49), ("rpm", 0, 1, 1, "cf2x", 1, 50), ("rpm", 0, 1, 1, "cf2x", 300, 64),
    ("rpm", 0, 1, 1, "cf2x", 1000, 47),
]


@pytest.mark.parametrize("keep_term", [True, False])
@pytest.mark.parametrize("act,flags,D,S,model,E,K", [c + (1536 // c[2], 24) for c in CASES] + RAGGED)
def test_rollout_is_bitwise_k_steps(gpu_device, act, flags, D, S, model, E, K, keep_term, scramble=False):
    """Same state, same actions: one rollout of K steps == K single-step launches, bit for bit, including the
    same-step auto-reset (short episodes so that resets happen inside the rollout), the terminal observations,
    the DSLPID members, last RPMs and step counters.  `keep_term` selects the kernel: single-drone aviaries without
    terminal observations and without DSLPID run `gpd_rollout1_kernel` (no helper wave; lanes of a ragged last
    workgroup are clones of the first drone of that workgroup), everything else the compute-wave + store-wave kernel."""
    rng = np.random.default_rng(zlib.crc32(repr((act, flags, D, S, model)).encode()))
    a, b = _pair(act, flags, D, S, model, gpu_device, E, rng, keep_term=keep_term)
    for c in (a, b):   # episodes of 10 physics steps -> several resets within K steps
        c._cfg.trunc_counter = 10
    if scramble:
        _scramble_arguments(np.random.default_rng(77), a, b)
    # give the state some velocity so the PID memories / drag see non-trivial values
    kin = a.kin.clone()
    kin[7:13] = torch.as_tensor(rng.uniform(-0.5, 0.5, size=(6, a.ld)), dtype=torch.float32, device=gpu_device)
    a.set_state(kin=kin[:, :a.N]); b.set_state(kin=kin[:, :b.N])
    acts = torch.as_tensor(_actions(rng, act, (K, E, D), a.P.HOVER_RPM).astype(np.float32), device=gpu_device)
    te_s, tr_s = rollout_equals_steps(a, b, acts, keep_term)
    assert act == "raw_rpm" or K * S <= 10 or tr_s.any(), "test must exercise the auto-reset"


def _scramble_arguments(rng, *cores):
    """Every float word of GpdParams and the float bounds of GpdStepCfg get a factor of their own (the same on every core)."""
    import ctypes
    words = ctypes.sizeof(cores[0]._params) // 4
    fac = rng.uniform(0.9, 1.1, size=words).astype(np.float32)
    cf = rng.uniform(0.7, 1.3, size=4)
    for c in cores:
        w = np.frombuffer((ctypes.c_char * (4 * words)).from_address(ctypes.addressof(c._params)), dtype=np.float32)
        w[1:] *= fac[1:]                      # (word 0 is the integer airframe code)
        for k, name in enumerate(("xy_bound", "z_bound", "tilt_bound", "term_dist")):
            setattr(c._cfg, name, getattr(c._cfg, name) * cf[k])


@pytest.mark.parametrize("keep_term", [True, False])
@pytest.mark.parametrize("act,flags,D,S,model", CASES)
def test_rollout_is_bitwise_with_every_argument_word_distinct(gpu_device, act, flags, D, S, model, keep_term):
    """The same comparison with every float of the by-value kernel arguments scaled by a factor of its own: the kernels are
    compiled separately (three kernel families, ~130 instantiations, 106 SGPRs full and kernel arguments spilled to VGPR lanes
    in all of them) and must have read the SAME word for every field -- which the shipped constants, full of equal values,
    cannot show.  (Not a physical airframe any more; nothing here is compared with the oracle.)"""
    test_rollout_is_bitwise_k_steps(gpu_device, act, flags, D, S, model, 1536 // D, 24, keep_term, scramble=True)


def test_rollout_strides_zero(gpu_device):
    """action stride 0 (hold one action) and last_only outputs."""
    rng = np.random.default_rng(3)
    E, K = 4096, 16
    a, b = _pair("pid", 0, 1, 2, "cf2x", gpu_device, E, rng, auto_reset=False, keep_term=False)
    act = torch.as_tensor(_actions(rng, "pid", (E, 1), a.P.HOVER_RPM).astype(np.float32), device=gpu_device)
    for _ in range(K):
        a.step(act)
    b.rollout(act, num_steps=K, last_only=True)
    for name in ("kin", "last_rpm", "pid", "step_counter", "obs12", "reward", "terminated", "truncated"):
        assert torch.equal(getattr(a, name), getattr(b, name)), name


@pytest.mark.parametrize("act,flags,D,S", [("rpm", 0, 1, 8), ("pid", 7, 4, 1)])
def test_rollout_against_oracle(gpu_device, act, flags, D, S):
    """K-step rollout vs the float64 oracle stepped K times (north-star metric, < 1e-4)."""
    rng = np.random.default_rng(17 + D)
    E, K = 2048 // D, 30
    task = "hover" if D == 1 else "multihover"
    xyz, rpy = _random_scene(rng, E, D)
    if D > 1:   # keep the downwash Gaussian well-conditioned (see test_open_loop_with_all_force_terms)
        xyz = rng.uniform(-0.02, 0.02, size=(E, D, 3)) + np.arange(D)[None, :, None] * np.array([0.12, 0.0, 0.3]) + \
            np.array([0, 0, 0.8])
        rpy = rng.uniform(-0.05, 0.05, size=(E, D, 3))
    orc = BatchedAviary(urdf("cf2x"), "cf2x", num_envs=E, num_drones=D, initial_xyzs=xyz, initial_rpys=rpy,
                        physics_flags=flags, pyb_freq=240, ctrl_freq=240 // S, act=act, task=task,
                        pid_urdf_path=urdf("cf2x"))
    core = _core("cf2x", E, D, flags, S, act, task, xyz, rpy, gpu_device, target=orc.TARGET_POS)
    _sync_from_oracle(core, orc)
    if act == "pid":
        acts = (xyz + np.array([0, 0, 0.2]) + 0.05 * rng.uniform(-1, 1, size=(K, E, D, 3))).astype(np.float32)
    else:
        acts = (0.02 * rng.uniform(-1, 1, size=(K, E, D, 4))).astype(np.float32)
    obs, rew, te, tr = core.rollout(torch.as_tensor(acts, device=gpu_device))
    o64 = []
    r64 = []
    for k in range(K):
        o, r, _, _, _ = orc.step(acts[k].astype(np.float64))
        o64.append(o.reshape(E * D, 12)); r64.append(r)
    o64, r64 = np.stack(o64), np.stack(r64)
    o32 = obs.cpu().numpy().astype(np.float64)
    scale = np.maximum(np.abs(o64).max(axis=(0, 1)), 1.0)
    err = np.abs(o32 - o64) / scale
    print("obs12 col err", err.max(axis=(0, 1)))
    assert err.max() < 1e-4
    np.testing.assert_allclose(rew.cpu().numpy(), r64, rtol=1e-4, atol=1e-4)
    kin = core.kin[:, :E * D].cpu().numpy().astype(np.float64)
    ref = _oracle_kin(orc)
    assert (np.abs(kin - ref) / np.maximum(np.abs(ref).max(axis=1, keepdims=True), 1.0)).max() < 1e-4
    np.testing.assert_array_equal(core.step_counter.cpu().numpy(), orc.step_counter)


@pytest.mark.parametrize("act,D,ctrl", [("rpm", 1, 30), ("pid", 2, 48), ("one_d_rpm", 1, 240)])
def test_full_observation_rows_step_vs_rollout(gpu_device, act, D, ctrl):
    """The (12 + H*A) observation rows (kinematics + the last H actions, oldest first, BaseRLAviary.py:307-320)
    assembled after K single steps and after rollouts of the same actions are identical; the history survives
    resets and spans the boundary between two rollouts."""
    from gym_pybullet_drones_amd.envs import VectorAviary
    from gym_pybullet_drones_amd.utils.enums import ActionType
    rng = np.random.default_rng(5)
    E, K = 300, 7
    mk = lambda: VectorAviary(E, D, act=ActionType(act), ctrl_freq=ctrl, task="hover" if D == 1 else "multihover",  # noqa: E731
                              full_obs=True, auto_reset=True, episode_len_sec=0.05, device=gpu_device)
    a, b = mk(), mk()
    H, A = a.ACTION_BUFFER_SIZE, a.ACT_DIM
    acts = torch.as_tensor(rng.uniform(-1, 1, size=(2 * K, E, D, A)).astype(np.float32), device=gpu_device)
    rows = []
    for k in range(2 * K):
        o, *_ = a.step(acts[k])
        rows.append(o.clone())
    rows = torch.stack(rows)
    o1 = b.rollout(acts[:K])[0].clone()          # (rollout outputs are persistent buffers, overwritten by the next call)
    o2, *_ = b.rollout(acts[K:])
    assert o1.shape == (K, E, D, 12 + H * A)
    assert torch.equal(torch.cat([o1, o2]), rows)
    # the tail is exactly the sent actions (zeros before the first step)
    tail = rows[-1][..., 12:].reshape(E, D, H, A).cpu().numpy()
    sent = acts.cpu().numpy()
    for h in range(H):
        idx = 2 * K - 1 - (H - 1) + h
        want = sent[idx] if idx >= 0 else np.zeros((E, D, A), dtype=np.float32)
        np.testing.assert_array_equal(tail[:, :, h, :], want)
    assert torch.equal(a.action_history(), b.action_history())


@pytest.mark.parametrize("act,D,ctrl,E,K,fused", [("rpm", 1, 240, 1000, 7, True), ("rpm", 1, 30, 333, 40, True), ("pid", 1, 48, 300, 30, True),
                                                  ("one_d_rpm", 2, 30, 257, 20, True), ("vel", 4, 240, 130, 9, True), ("rpm", 3, 48, 100, 12, True),
                                                  ("pid", 7, 48, 41, 12, True), ("rpm", 70, 48, 5, 12, False)])
def test_rollout_with_lazy_history_pushes_the_ring_inside_the_kernel(gpu_device, act, D, ctrl, E, K, fused, scene=None):
    """`gpd_rollout_history` (VectorAviary(full_obs="lazy").rollout): every step's action goes into the action ring inside the
    rollout kernel.  Same observations, same ring (the zero-copy history view, the ring positions), same continuation as K
    single steps -- for rollouts shorter and longer than the history, ragged batches, aviaries of 2, 3, 4 and 7 drones (whole
    aviaries per wave: 63 of a wave's lanes hold a drone for 3 and 7); an aviary of 70 drones has no fused variant and takes the
    post-pass (`pushed_history` False), with the same result.
    `scene` (tests/test_gpu_aviary_sizes.py): constructor arguments on top of these, and the z_bound of the two cores."""
    from gym_pybullet_drones_amd.envs import VectorAviary
    from gym_pybullet_drones_amd.utils.enums import ActionType
    rng = np.random.default_rng(K)
    kw, z_bound = scene or ({}, None)
    mk = lambda: VectorAviary(E, D, act=ActionType(act), ctrl_freq=ctrl, task="hover" if D == 1 else "multihover",  # noqa: E731
                              full_obs="lazy", auto_reset=True, episode_len_sec=0.1, device=gpu_device, **kw)
    a, b = mk(), mk()
    A = a.ACT_DIM
    # (every float of the kernel arguments scaled by a factor of its own: the fused variants are instantiations of their own,
    # with their own register allocation -- see test_rollout_is_bitwise_with_every_argument_word_distinct)
    _scramble_arguments(np.random.default_rng(79), a.core, b.core)
    if z_bound is not None:                  # (after the scaling: above the column whatever its factor)
        a.core._cfg.z_bound = b.core._cfg.z_bound = z_bound
    acts = torch.as_tensor(rng.uniform(-1, 1, size=(2 * K + 3, E, D, A)).astype(np.float32), device=gpu_device)
    for k in range(3):                       # some history first
        a.step(acts[k]); b.step(acts[k])
    rows, flags = [], []
    for k in range(3, 3 + 2 * K):
        o, r, te, tr, _ = a.step(acts[k])
        rows.append(o.clone()); flags.append((r.clone(), te.clone(), tr.clone()))
    o1, r1, te1, tr1 = (x.clone() for x in b.rollout(acts[3:3 + K]))
    assert b.core.pushed_history == fused
    h_mid = b.history().clone()
    o2, r2, te2, tr2 = b.rollout(acts[3 + K:])
    assert torch.equal(torch.cat([o1, o2]), torch.stack(rows))
    for k, (r, te, tr) in enumerate(flags):
        assert torch.equal(r, (r1 if k < K else r2)[k % K]) and torch.equal(te, (te1 if k < K else te2)[k % K]) and \
            torch.equal(tr, (tr1 if k < K else tr2)[k % K]), k
    assert torch.stack([f[2] for f in flags]).any() or 2 * K + 3 < 0.1 * ctrl or act in ("pid", "vel"), "the test should see episodes end"
    assert scene is None or not torch.stack([f[2] for f in flags]).all(), "... and not at every step"
    assert torch.equal(a.history(), b.history()) and torch.equal(a.core.ring_pos, b.core.ring_pos)
    assert torch.equal(a.core.act_ring, b.core.act_ring)
    # the view after the first rollout ends with that rollout's last actions, oldest first
    H = a.ACTION_BUFFER_SIZE
    sent = acts[:3 + K].cpu().numpy()
    tail = h_mid.cpu().numpy().reshape(E, D, H, A)
    for h in range(H):
        idx = 3 + K - 1 - (H - 1) + h
        np.testing.assert_array_equal(tail[:, :, h, :], sent[idx] if idx >= 0 else np.zeros((E, D, A), dtype=np.float32))
    o, *_ = a.step(acts[0]); p, *_ = b.step(acts[0])          # and stepping goes on from the same ring
    assert torch.equal(o, p) and torch.equal(a.history(), b.history())


def test_rollout_arena_places_the_blocks_and_changes_no_bit(gpu_device):
    """`placement.RolloutArena` (at millions of drones the launch's rate follows the physical placement of its blocks,
    so the library carves them out of one arena at offsets it chooses by probing with the launch itself): at a size a test can afford
    the search runs its probes, installs the winning blocks as the core's rollout buffers, the action view lives inside the arena, and
    a rollout through the arena is bit for bit the rollout of a core with ordinary buffers.  Candidate layouts: inside the arena,
    disjoint, no duplicates (`layout_candidates`, also checked without a GPU in tests/test_host_logic.py)."""
    from gym_pybullet_drones_amd.envs import VectorHoverAviary
    from gym_pybullet_drones_amd.placement import RolloutArena, layout_candidates, place_rollout
    from gym_pybullet_drones_amd.utils.enums import ActionType
    E, K = 16384, 16
    rng = np.random.default_rng(5)
    a = VectorHoverAviary(E, act=ActionType.RPM, ctrl_freq=240, auto_reset=True, device=gpu_device)
    b = VectorHoverAviary(E, act=ActionType.RPM, ctrl_freq=240, auto_reset=True, device=gpu_device)
    arena = RolloutArena(a.core, K, arena_bytes=256 << 20, grid_bytes=16 << 20)
    cand = arena.candidates()
    assert len(cand) == len(set(cand)) > 50
    assert all(h + arena.head_bytes <= arena.bytes and t + arena.tail_bytes <= arena.bytes and
               (t + arena.tail_bytes <= h or t >= h + arena.head_bytes) for h, t in cand)
    rep = arena.search(target=2.0, max_probes=6)          # an unreachable target: all six probes run, the best one is installed
    assert rep["probes"] == 6 and not rep["reached_target"] and 0 < rep["best_frac_in_search"] < 1.5 and len(rep["all_probes"]) == 6
    lo, hi = arena.slab.data_ptr(), arena.slab.data_ptr() + arena.bytes
    obs_buf = a.core._rollout_cache[K][0]
    assert lo <= obs_buf.data_ptr() < hi and lo <= arena.actions.data_ptr() < hi and arena.actions.shape == (K, E, 4)
    assert arena.layout == (int(rep["obs_at_gib"] * 2 ** 30), int(rep["tail_at_gib"] * 2 ** 30))
    a.reset(); b.reset()
    acts = torch.as_tensor(rng.uniform(-1, 1, size=(K, E, 1, 4)).astype(np.float32), device=gpu_device)
    arena.actions.copy_(acts.view(K, E, 4))
    for _ in range(3):
        oa = a.core.rollout(arena.actions)
        ob = b.core.rollout(acts)
        assert oa[0].data_ptr() == obs_buf.data_ptr()                    # the arena's blocks ARE the rollout buffers
        assert all(torch.equal(x, y) for x, y in zip(oa, ob)) and torch.equal(a.core.kin_store, b.core.kin_store)
    arena2, rep2 = place_rollout(b.core, K, target=0.0, max_arenas=2, max_probes=4)       # a target every layout reaches: one confirmed probe
    assert rep2["probes"] == 1 and rep2["arenas_tried"] == 1 and rep2["reached_target"] and "confirmed_frac" in rep2["all_probes"][0]
    assert b.core._rollout_cache[K][0].data_ptr() >= arena2.slab.data_ptr()


def test_kernels_compiled_for_one_aviary_size_and_flag_set_are_the_generic_kernels_bit_for_bit():
    """`gpd_rollout1_kernel` / `gpd_step_kernel` have variants with the aviary size, the physics flags and "one sub-step per step" as
    template parameters (BASELINE configs 3 (i), 3 (ii), 5 run 12 / 26 / 28 % faster with them).  Same operations,
    same order: rollouts and single steps of thirty shapes (aviaries of 16, 33 and 64 drones among them), and four rollouts that keep terminal observations (the third kernel's variants) -- every variant, and shapes that fall through to the generic kernels --
    digest identically with GPD_ROLLOUT_SIZED=0 (generic kernels only; the switch is read once per process, hence the two children)."""
    import json
    import os
    import subprocess
    import sys
    here = os.path.dirname(os.path.abspath(__file__))
    got = {}
    for label, extra in (("generic", {"GPD_ROLLOUT_SIZED": "0"}), ("sized", {})):
        env = {k: v for k, v in os.environ.items() if k != "GPD_ROLLOUT_SIZED"}
        res = subprocess.run([sys.executable, os.path.join(here, "helpers", "sized_digests.py")], env=dict(env, **extra), capture_output=True,
                             text=True, timeout=600)
        line = next((l for l in res.stdout.splitlines() if l.startswith("{")), None)
        assert res.returncode == 0 and line, res.stderr[-1500:]
        got[label] = json.loads(line)
    assert len(got["generic"]) == 34 and got["generic"] == got["sized"], {k: (v, got["sized"].get(k)) for k, v in got["generic"].items() if got["sized"].get(k) != v}
