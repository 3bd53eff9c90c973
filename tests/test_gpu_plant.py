"""The per-drone plant (domain randomisation: `SimCore.set_plant`, `VectorAviary(randomize=...)`, include/gpd.h GPD_PLANT_*) on an
MI355X: the derivation of the rows, bit-identity of an all-ones table with the uniform kernels, the physics of every scaled field
against the float64 oracle, the indexing of heterogeneous rows, and the invariants the uniform path already keeps."""
import ctypes
import zlib

import numpy as np
import pytest
import torch

from test_gpu_parity import _check_single_steps, _oracle_and_core, _sync_from_oracle

pytestmark = pytest.mark.gpu

ACT = {"rpm": 0, "pid": 1, "vel": 2, "one_d_rpm": 3, "one_d_pid": 4, "raw_rpm": 5, "direct_rpm": 6}
NF = 9


def _core(dev, act, flags, D, S, E, auto_reset=True, keep_term=False, episode=0.15, seed=0):
    from gym_pybullet_drones_amd import engine
    from gym_pybullet_drones_amd.utils.enums import DroneModel
    rng = np.random.default_rng(seed)
    xyz = np.zeros((E, D, 3))
    xyz[..., :2] = rng.uniform(-0.3, 0.3, size=(E, D, 2))
    xyz[..., 2] = (0.05 if flags & 8 else 0.4) + 0.3 * np.arange(D) + rng.uniform(-0.02, 0.02, size=(E, D))
    rpy = rng.uniform(-0.1, 0.1, size=(E, D, 3))
    task = engine.TASK_NONE if act in ("raw_rpm", "direct_rpm") else (engine.TASK_HOVER if D == 1 else engine.TASK_MULTIHOVER)
    return engine.SimCore(drone_model=DroneModel.CF2X, num_envs=E, drones_per_env=D, physics=flags, pyb_freq=240, ctrl_freq=240 // S,
                          act_code=ACT[act], task=task, initial_xyzs=xyz, initial_rpys=rpy, target_pos=np.zeros((D, 3)) + [0, 0, 0.5],
                          episode_len_sec=episode, auto_reset=auto_reset, track_rpm=True, keep_terminal_obs=keep_term, device=dev)


def _actions(core, act, calls, seed=1):
    g = torch.Generator(device=core.device)
    g.manual_seed(seed)
    a = torch.rand((calls, core.N, core.A), generator=g, device=core.device) * 2 - 1
    if act in ("pid",):
        a = a * 0.3 + torch.tensor([0.0, 0.0, 0.5], device=core.device)
    elif act in ("raw_rpm", "direct_rpm"):
        a = float(core.P.HOVER_RPM) * (1 + 0.1 * a)
    return a.contiguous()


def _bits(t):
    t = t.contiguous()
    return t.view(torch.int32) if t.dtype == torch.float32 else t.view(torch.uint8)


def _state(core):
    out = [core.kin_store, core.step_counter, core.last_rpm]
    if core.pid is not None:
        out.append(core.pid)
    return [_bits(t).clone() for t in out]


def _drive(core, act, K, calls, seed=1):
    """`calls` launches of K steps (K = 1: step()); every output of every call and the final state, as bit patterns"""
    acts = _actions(core, act, calls * K, seed)
    outs = []
    for c in range(calls):
        if K == 1:
            o = core.step(acts[c])
            outs += [_bits(x).clone() for x in o]
            if core.term_obs12 is not None:
                outs.append(_bits(core.term_obs12).clone())
        else:
            o = core.rollout(acts[c * K:(c + 1) * K])
            outs += [_bits(x).clone() for x in o]
            if core.term_obs12 is not None:
                outs.append(_bits(core.terminal_observations(K)).clone())
    torch.cuda.synchronize()
    return outs, _state(core)


def _ref_rows(P, scales):
    """numpy float64 restatement of gpd_plant_derive (include/gpd.h GPD_PLANT_*), rounded once to fp32: [19, n]"""
    f = lambda v: float(np.float32(v))      # noqa: E731  (the nominal struct's fp32 fields)
    s = scales.astype(np.float64)
    m, kf, ht = s[0], s[4], f(P.hover_thrust)
    rows = [f(P.M) * m, f(P.inv_M) / m, f(P.KF) * kf, f(P.GRAVITY) * m]
    rows += [f(P.J[k]) * s[1 + k] for k in range(3)] + [f(P.J_INV[k]) / s[1 + k] for k in range(3)]
    rows += [f(P.km_over_kf) * s[5] / kf, f(P.gnd_eff_coeff) * s[8]]
    rows += [f(P.drag_coeff[0]) * s[6], f(P.drag_coeff[1]) * s[6], f(P.drag_coeff[2]) * s[7]]
    rows += [ht * m, f(P.hover_resid) * kf + (kf - m) * ht, ht * kf, (m - kf) * ht]
    return np.stack(rows).astype(np.float32)


def _derive(lib, P, scales_t, rows_t, E, D, ld, mask=None):
    from gym_pybullet_drones_amd import _native
    rc = lib.gpd_plant_derive(ctypes.byref(P), ctypes.c_void_p(scales_t.data_ptr()),
                              ctypes.c_void_p(mask.data_ptr() if mask is not None else 0), E, D, ld, ctypes.c_void_p(rows_t.data_ptr()), None)
    _native.check(rc, "gpd_plant_derive")
    torch.cuda.synchronize()


@pytest.mark.parametrize("model", ["cf2x", "cf2p", "racer"])
def test_derive_reproduces_the_nominal_struct_and_the_float64_reference(gpu_device, model):
    from gym_pybullet_drones_amd import _native
    from gym_pybullet_drones_amd.params import DroneParams
    from gym_pybullet_drones_amd.utils.enums import DroneModel
    lib = _native.lib()
    P = DroneParams(DroneModel(model)).to_struct(pid_model=DroneModel.CF2X)
    E, D = 300, 3
    n, ld = E * D, 1024
    rows = torch.full((_native.PLANT_ROWS, ld), -7.0, device=gpu_device)
    ones = torch.ones((NF, ld), device=gpu_device)
    _derive(lib, P, ones, rows, E, D, ld)
    got = rows[:, :n].cpu().numpy()
    # all scales 1.0: to_struct's fields bit for bit (the two new rows: hover_thrust, and +0)
    want = []
    for name in _native.PLANT_ROW_FIELDS[:17]:
        base, _, idx = name.partition("[")
        v = getattr(P, base)
        want.append(v[int(idx[:-1])] if idx else v)
    want += [P.hover_thrust, 0.0]
    want = np.array(want, dtype=np.float32)
    assert np.array_equal(got.view(np.int32), np.broadcast_to(want[:, None], got.shape).view(np.int32))
    assert (rows[:, n:] == -7.0).all()                                  # nothing beyond n drones
    # random scales in [0.7, 1.3]: the numpy float64 reference rounded once, bit for bit
    rng = np.random.default_rng(zlib.crc32(model.encode()))
    sc = rng.uniform(0.7, 1.3, size=(NF, n)).astype(np.float32)
    st = torch.ones((NF, ld), device=gpu_device)
    st[:, :n] = torch.as_tensor(sc, device=gpu_device)
    _derive(lib, P, st, rows, E, D, ld)
    assert np.array_equal(rows[:, :n].cpu().numpy().view(np.int32), _ref_rows(P, sc).view(np.int32))
    # masked: the rows of the other aviaries are untouched
    rows.fill_(-7.0)
    mask = torch.as_tensor(rng.uniform(size=E) < 0.4, device=gpu_device).to(torch.uint8)
    _derive(lib, P, st, rows, E, D, ld, mask)
    sel = np.repeat(mask.cpu().numpy().astype(bool), D)
    got = rows[:, :n].cpu().numpy()
    assert (got[:, ~sel] == -7.0).all() and sel.any() and (~sel).any()
    assert np.array_equal(got[:, sel].view(np.int32), _ref_rows(P, sc)[:, sel].view(np.int32))


# (action, physics flags, drones per aviary, sub-steps, K, keep_terminal_obs): every action type, flags {0, 7, 8, 24, 31}, D {1, 2, 3, 8, 100},
# S {1, 8}, K {1, 20}, with and without terminal observations, auto-reset on and episodes short enough to end inside the horizon.  Between
# them, the PLANT = true instantiations of gpd_step_kernel (K = 1, single and multi), gpd_rollout1_kernel (K > 1, single and multi) and
# gpd_rollout_kernel (terminal observations, D > 64; single and multi)
NOMINAL_SHAPES = [("rpm", 0, 1, 1, 20, False), ("rpm", 0, 1, 1, 1, False), ("pid", 7, 2, 8, 20, False), ("vel", 8, 3, 1, 1, True),
                  ("one_d_rpm", 24, 8, 8, 20, True), ("one_d_pid", 31, 100, 1, 20, False), ("raw_rpm", 31, 1, 8, 20, True),
                  ("direct_rpm", 7, 100, 1, 1, False), ("one_d_pid", 24, 1, 8, 1, False), ("vel", 0, 2, 1, 20, False),
                  # the lane maps of larger aviaries: 33 drones (31 pad lanes per wave in gpd_rollout1_kernel, 231-lane workgroups in
                  # gpd_step_kernel) and 64 (full waves, groups of four mates), two workgroups with a ragged last one
                  ("rpm", 7, 33, 1, 20, False), ("pid", 7, 33, 2, 1, False), ("one_d_rpm", 31, 64, 1, 20, False), ("rpm", 7, 64, 8, 1, False)]


@pytest.mark.parametrize("act,flags,D,S,K,keep", NOMINAL_SHAPES)
def test_all_ones_table_is_the_uniform_path_bit_for_bit(gpu_device, act, flags, D, S, K, keep):
    E = {1: 300, 2: 150, 3: 150, 8: 40, 100: 6, 33: 9, 64: 5}[D]
    calls = 3 if K > 1 else (45 if S == 1 else 8)            # (episodes of 36 physics steps: every horizon spans auto-resets)
    a = _core(gpu_device, act, flags, D, S, E, keep_term=keep)
    b = _core(gpu_device, act, flags, D, S, E, keep_term=keep)
    b.set_plant(torch.ones((NF, E), device=gpu_device))
    assert b.plant_rows is not None and a.plant_rows is None
    if D in (33, 64):          # (z_bound above the stack: these aviaries end by time, not at every step)
        a._cfg.z_bound = b._cfg.z_bound = 0.4 + 0.3 * D + 1.0
    oa, sa = _drive(a, act, K, calls)
    ob, sb = _drive(b, act, K, calls)
    assert len(oa) == len(ob)
    for i, (x, y) in enumerate(zip(oa + sa, ob + sb)):
        assert torch.equal(x, y), f"output {i} differs"


SCALES = {"mass": 1.22, "ixx": 0.81, "iyy": 1.17, "izz": 0.76, "kf": 1.13, "km": 0.84, "drag_xy": 1.28, "drag_z": 0.73, "gnd_eff": 1.25}


def _scale_oracle(b, s):
    C = b.C
    C.M = C.M * s["mass"]
    C.GRAVITY = C.G * C.M
    J = np.diag(np.diag(C.J) * np.array([s["ixx"], s["iyy"], s["izz"]]))
    C.J, C.J_INV = J, np.linalg.inv(J)
    C.KF, C.KM = C.KF * s["kf"], C.KM * s["km"]
    C.DRAG_COEFF = C.DRAG_COEFF * np.array([s["drag_xy"], s["drag_xy"], s["drag_z"]])
    C.GND_EFF_COEFF = C.GND_EFF_COEFF * s["gnd_eff"]          # (HOVER_RPM, MAX_RPM and the controller stay nominal)


@pytest.mark.parametrize("act,flags,D", [("rpm", 0, 1), ("rpm", 31, 2), ("pid", 7, 1), ("pid", 0, 2), ("vel", 31, 1), ("vel", 7, 2),
                                         ("one_d_rpm", 7, 1), ("one_d_rpm", 0, 2), ("raw_rpm", 31, 2), ("raw_rpm", 0, 1)])
def test_each_scaled_field_against_the_float64_oracle(gpu_device, act, flags, D):
    """The setup of test_gpu_parity's perturbed-constants test: the oracle's plant constants are scaled, its HOVER_RPM / MAX_RPM /
    controller are not; the core keeps its nominal GpdParams and gets the same scales through the table."""
    S = 1
    rng = np.random.default_rng(zlib.crc32(repr(("plant", act, flags, D)).encode()))
    b, core = _oracle_and_core(rng, "cf2x", act, flags, D, S, gpu_device)
    _scale_oracle(b, SCALES)
    core.set_plant({k: v for k, v in SCALES.items()})
    _check_single_steps(rng, b, core, act, flags, gpu_device)
    # ... and the table is read: one step from the same state with and without it differs by far more than the tolerance (2e-5)
    _sync_from_oracle(core, b)
    snap = core.get_state()
    snap.pop("plant_scales")
    from test_gpu_parity import _actions as parity_actions
    a = torch.as_tensor(parity_actions(rng, act, (b.E, b.D), b.C.HOVER_RPM).astype(np.float32), device=gpu_device)
    core.step(a)
    k_plant = core.kin[:, :core.N].clone()
    core.set_state(**snap)
    core.clear_plant()
    core.step(a)
    k_nom = core.kin[:, :core.N].clone()
    scale = torch.clamp(k_nom.abs().amax(dim=1, keepdim=True), min=1.0)
    assert float(((k_plant - k_nom).abs() / scale).max()) > 1e-3


def _rows_table(dev, E, D, per_env_rows):
    """[9, E, D] from per-aviary rows [E, 9] (or per drone [E, D, 9])"""
    t = torch.as_tensor(np.array(per_env_rows), dtype=torch.float32, device=dev)
    if t.ndim == 2:
        t = t[:, None, :].expand(E, D, NF)
    return t.permute(2, 0, 1).contiguous()


@pytest.mark.parametrize("K", [1, 20])
def test_heterogeneous_rows_index_by_aviary(gpu_device, K):
    """70 aviaries of two drones with downwash and auto-reset, seven distinct airframes (aviary e flies row e % 7): every aviary's
    outputs and state equal, bit for bit, those of a run whose table holds its row everywhere."""
    E, D = 70, 2
    rng = np.random.default_rng(5)
    distinct = rng.uniform(0.75, 1.3, size=(7, NF))
    calls = 2 if K > 1 else 25

    def run(rows_of_env):
        core = _core(gpu_device, "rpm", 7, D, 1, E)
        core.set_plant(_rows_table(gpu_device, E, D, rows_of_env))
        outs, st = _drive(core, "rpm", K, calls)
        return core, outs, st

    het_core, het, het_state = run(distinct[np.arange(E) % 7])
    kin_h = het_core.kin[:, :E * D].view(13, E, D)
    for j in range(7):
        core, uni, _ = run(np.broadcast_to(distinct[j], (E, NF)))
        envs = torch.arange(E, device=gpu_device)[torch.arange(E, device=gpu_device) % 7 == j]
        for x, y in zip(het, uni):
            if x.numel() == E * K or x.numel() == E:                 # reward / flags: [K, E] or [E]
                xv, yv = x.view(-1, E), y.view(-1, E)
            else:                                                    # observation rows: [.., E * D, 12]
                xv, yv = x.view(-1, E, D * 12), y.view(-1, E, D * 12)
            assert torch.equal(xv[:, envs], yv[:, envs]), j
        kin_u = core.kin[:, :E * D].view(13, E, D)
        assert torch.equal(_bits(kin_h[:, envs]), _bits(kin_u[:, envs])), j


def test_heterogeneous_rows_index_by_drone(gpu_device):
    """Inside an aviary (two drones, no downwash, no auto-reset, a horizon short of truncation): each drone's kinematics equal those of
    the run where both drones carry its row."""
    E, D = 64, 2
    rng = np.random.default_rng(6)
    per_drone = rng.uniform(0.75, 1.3, size=(E, D, NF))

    def run(table):
        core = _core(gpu_device, "rpm", 0, D, 1, E, auto_reset=False, episode=8.0)
        core.set_plant(_rows_table(gpu_device, E, D, table))
        _drive(core, "rpm", 20, 1)
        _drive(core, "rpm", 1, 5, seed=2)
        return core.kin[:, :E * D].view(13, E, D).clone()

    k = run(per_drone)
    for d in range(D):
        kd = run(np.broadcast_to(per_drone[:, d:d + 1, :], (E, D, NF)))
        assert torch.equal(_bits(k[:, :, d]), _bits(kd[:, :, d])), d


@pytest.mark.parametrize("act,flags,D,S,keep", [("rpm", 7, 1, 1, False), ("pid", 31, 3, 8, False), ("one_d_rpm", 24, 2, 1, True)])
def test_rollout_equals_single_steps_with_a_perturbed_table(gpu_device, act, flags, D, S, keep):
    E, K = 128, 20
    rng = np.random.default_rng(7)
    table = rng.uniform(0.75, 1.3, size=(E, D, NF))
    a = _core(gpu_device, act, flags, D, S, E, keep_term=keep)
    b = _core(gpu_device, act, flags, D, S, E, keep_term=keep)
    for c in (a, b):
        c.set_plant(_rows_table(gpu_device, E, D, table))
    acts = _actions(a, act, K)
    obs, rew, term, trunc = a.rollout(acts)
    for t in range(K):
        o, r, te, tr = b.step(acts[t])
        assert torch.equal(_bits(obs[t]), _bits(o)) and torch.equal(_bits(rew[t]), _bits(r)), t
        assert torch.equal(te, term[t]) and torch.equal(tr, trunc[t]), t
    assert all(torch.equal(x, y) for x, y in zip(_state(a), _state(b)))


def test_state_snapshot_carries_the_airframes(gpu_device):
    E, D, act = 96, 2, "vel"
    rng = np.random.default_rng(8)
    a = _core(gpu_device, act, 7, D, 1, E)
    a.set_plant(_rows_table(gpu_device, E, D, rng.uniform(0.75, 1.3, size=(E, D, NF))))
    _drive(a, act, 1, 10)
    snap = a.get_state()
    assert tuple(snap["plant_scales"].shape) == (NF, E * D)
    outs_a, st_a = _drive(a, act, 20, 2, seed=3)
    b = _core(gpu_device, act, 7, D, 1, E)
    b.set_state(**snap)                                              # the airframes come with the snapshot, the rows are re-derived
    assert b.plant_rows is not None
    outs_b, st_b = _drive(b, act, 20, 2, seed=3)
    assert all(torch.equal(x, y) for x, y in zip(outs_a + st_a, outs_b + st_b))


def test_randomize_resamples_only_the_aviaries_that_ended_and_is_seeded(gpu_device):
    from gym_pybullet_drones_amd.envs import VectorHoverAviary
    kw = dict(ctrl_freq=240, episode_len_sec=0.05, randomize={"mass": 0.2, "kf": 0.1, "izz": 0.3}, device=gpu_device)
    E = 512
    env = VectorHoverAviary(E, **kw)
    env.reset(seed=11)
    p0 = env.physical_params().clone()
    assert tuple(p0.shape) == (E, 1, 9)
    assert (p0[..., 0] - 1).abs().max() <= 0.2 + 1e-6 and p0[..., 0].std() > 0.05 and (p0[..., 5] == 1).all()      # km not randomised
    g = torch.Generator(device=gpu_device)
    g.manual_seed(1)
    acts = torch.rand((20, E, 1, 4), generator=g, device=gpu_device) * 2 - 1
    ended_any = False
    prev = p0
    trace = []
    for t in range(20):
        obs, rew, term, trunc, _ = env.step(acts[t])
        cur = env.physical_params().clone()
        done = (term | trunc)
        changed = (cur != prev).any(dim=2).any(dim=1)
        assert not bool((changed & ~done).any()), t                  # only aviaries that ended fly new airframes ...
        assert bool((changed == done).all()), t                      # ... and every one of them does
        ended_any |= bool(done.any())
        prev = cur
        trace.append(_bits(obs).clone())
    assert ended_any
    # seeded: a second aviary with the same seed and actions flies the same airframes and trajectories
    env2 = VectorHoverAviary(E, **kw)
    env2.reset(seed=11)
    assert torch.equal(env2.physical_params(), p0)
    for t in range(20):
        obs, *_ = env2.step(acts[t])
        assert torch.equal(_bits(obs), trace[t]), t
    assert torch.equal(env2.physical_params(), prev)
    # a masked reset resamples the masked aviaries only
    mask = torch.zeros(E, dtype=torch.bool, device=gpu_device)
    mask[::3] = True
    before = env2.physical_params().clone()
    env2.reset(mask=mask)
    changed = (env2.physical_params() != before).any(dim=2).any(dim=1)
    assert torch.equal(changed, mask)


def test_policy_kernel_and_swarm_refuse_a_plant_table(gpu_device):
    from gym_pybullet_drones_amd import _native
    from gym_pybullet_drones_amd.policy import MlpPolicy
    core = _core(gpu_device, "rpm", 0, 1, 1, 64)
    core.set_plant({"mass": 1.1})
    pol = MlpPolicy.random(12, 4, device=gpu_device)
    with pytest.raises(_native.GpdError, match="plant"):
        core.rollout_policy(pol, 4)
    core.clear_plant()
    core.rollout_policy(pol, 4)                                      # (back to the nominal airframe: the policy kernel runs again)
    with pytest.raises(ValueError, match="finite and > 0"):
        core.set_plant({"kf": 0.0})
    with pytest.raises(ValueError, match="finite and > 0"):
        core.set_plant(torch.full((NF, 64), float("nan"), device=gpu_device))


def test_vector_env_adapters_pass_the_randomised_plant_through(gpu_device):
    """The SB3- and gymnasium-shaped front ends need nothing of their own: the aviaries that end inside their step are resampled, and
    gymnasium's reset(seed=) seeds the airframes."""
    from gym_pybullet_drones_amd.envs import VectorHoverAviary
    from gym_pybullet_drones_amd.envs.VectorAviary import GymVectorEnvAdapter, VecEnvAdapter
    kw = dict(ctrl_freq=240, episode_len_sec=0.05, randomize={"mass": 0.2, "kf": 0.1}, device=gpu_device)
    E = 64
    firsts = []
    for _ in range(2):
        g = GymVectorEnvAdapter(VectorHoverAviary(E, **kw))
        g.reset(seed=5)
        firsts.append(g.env.physical_params().clone())
        p0 = firsts[-1]
        ended = np.zeros(E, dtype=bool)
        for _ in range(15):                                          # episodes of 12 steps: every aviary ends once
            _, _, term, trunc, _ = g.step(np.zeros((E, 4), dtype=np.float32))
            ended |= np.asarray(term, dtype=bool) | np.asarray(trunc, dtype=bool)
        changed = (g.env.physical_params() != p0).any(dim=2).any(dim=1).cpu().numpy()
        assert ended.all() and np.array_equal(changed, ended)
    assert torch.equal(firsts[0], firsts[1])
    v = VecEnvAdapter(VectorHoverAviary(E, **kw))
    v.reset()
    p0 = v.env.physical_params().clone()
    done_any = np.zeros(E, dtype=bool)
    for _ in range(15):
        _, _, dones, infos = v.step(np.zeros((E, 1, 4), dtype=np.float32))
        done_any |= np.asarray(dones, dtype=bool)
    assert done_any.all() and bool((v.env.physical_params() != p0).any(dim=2).any(dim=1).all())
