"""The wider drop-in surface on the GPU: VelocityAviary against the reference's own run (fixture), the batched
VectorVelocityAviary, the SB3-VecEnv-shaped adapter, and Logger export of device state vectors."""
import numpy as np
import pytest
import torch

from conftest import golden

pytestmark = pytest.mark.gpu


def test_reference_fixture_velocity_aviary(gpu_device):
    """examples/pid_velocity.py scenario: the drop-in `VelocityAviary` (GPD_ACT_VEL fused in the kernel) against the
    reference's VelocityAviary(DYN), 4 drones, 48 Hz control / 240 Hz physics.  Tight while the DSLPID attitude loop
    has not yet amplified fp32 rounding (first 20 steps), bounded afterwards (chatter on the +-3200 torque clip)."""
    from gym_pybullet_drones_amd.envs import VectorVelocityAviary, VelocityAviary
    from gym_pybullet_drones_amd.utils.enums import DroneModel, Physics
    g = golden("velocity_aviary_cf2x")
    n, hz = g["init_xyzs"].shape[0], int(g["ctrl_hz"])
    env = VelocityAviary(drone_model=DroneModel.CF2X, num_drones=n, initial_xyzs=g["init_xyzs"], initial_rpys=g["init_rpys"],
                         physics=Physics.DYN, pyb_freq=240, ctrl_freq=hz, device=gpu_device)
    assert env.SPEED_LIMIT == pytest.approx(float(g["speed_limit"]))
    assert env.action_space.shape == (n, 4) and env.observation_space.shape == (n, 20)
    vec = VectorVelocityAviary(3, n, initial_xyzs=g["init_xyzs"], initial_rpys=g["init_rpys"], ctrl_freq=hz, device=gpu_device)
    obs0, info = env.reset()
    assert obs0.shape == (n, 20) and info == {"answer": 42}
    for k in range(g["obs"].shape[0]):
        obs, rew, term, trunc, info = env.step(g["actions"][k])
        vec.step(torch.as_tensor(np.broadcast_to(g["actions"][k], (3, n, 4)).astype(np.float32), device=gpu_device))
        assert rew == -1 and term is False and trunc is False
        ref = g["obs"][k]
        # rounding-level differences grow ~10x per 4 control steps in this loop (the body rates first) until they
        # saturate at the chatter amplitude: tight early, by field group; bounded later
        e = np.abs(obs - ref)
        if k < 12:
            assert e[:, 0:13].max() < 1e-5 and e[:, 13:16].max() < 1e-3 and e[:, 16:20].max() < 2.0, (k, e.max(axis=0))
        elif k < 24:
            assert e[:, 0:3].max() < 1e-4 and e[:, 3:10].max() < 3e-3 and e[:, 10:13].max() < 2e-3, (k, e.max(axis=0))
        else:
            assert e[:, 0:3].max() < 0.05, k
        # the batched class computes the same thing for each of its aviaries, bit for bit
        sv = vec.state_vectors().cpu().numpy()
        assert np.array_equal(sv[0], sv[2])
        np.testing.assert_array_equal(sv[1].astype(np.float64), obs)


def test_vecenv_adapter_follows_dummyvecenv(gpu_device):
    """numpy in/out, dones = terminated | truncated, same-step reset with info["terminal_observation"] and
    info["TimeLimit.truncated"] (what SB3's DummyVecEnv + Monitor give examples/learn.py)."""
    from gym_pybullet_drones_amd.envs import VecEnvAdapter, VectorHoverAviary
    from gym_pybullet_drones_amd.utils.enums import ActionType
    E = 64
    base = VectorHoverAviary(E, act=ActionType.ONE_D_RPM, ctrl_freq=30, full_obs=True, episode_len_sec=0.2, device=gpu_device)
    venv = VecEnvAdapter(base, squeeze=True)
    H = 15
    assert venv.num_envs == E and venv.observation_space.shape == (12 + H,) and venv.action_space.shape == (1,)
    obs = venv.reset()
    assert obs.shape == (E, 12 + H) and obs.dtype == np.float32
    rng = np.random.default_rng(0)
    seen_done = False
    for k in range(12):
        a = rng.uniform(-1, 1, size=(E, 1)).astype(np.float32)
        prev = obs
        obs, rew, dones, infos = venv.step(a)
        assert obs.shape == (E, 12 + H) and rew.shape == (E,) and dones.dtype == bool and len(infos) == E
        np.testing.assert_array_equal(obs[:, -1], a[:, 0])                 # newest action is the last history entry
        for i in np.flatnonzero(dones):
            seen_done = True
            t = infos[i]["terminal_observation"]
            assert t.shape == (12 + H,) and infos[i]["TimeLimit.truncated"] in (True, False)
            assert obs[i, 2] == pytest.approx(0.1125, abs=1e-6)            # returned obs: first one of the new episode
            assert t[2] != pytest.approx(0.1125, abs=1e-6) or abs(a[i, 0]) < 1e-3
        for i in np.flatnonzero(~dones):
            assert infos[i] == {}
    assert seen_done                                                        # 0.2 s episodes at 30 Hz: truncation on step 8
    assert venv.env_is_wrapped(object) == [False] * E and venv.get_attr("CTRL_FREQ")[0] == 30


def test_gymnasium_vector_env_adapter(gpu_device):
    """gymnasium >= 1.0 vector API: batched (obs, rewards, terminations, truncations, infos), SAME_STEP autoreset with
    infos["final_obs"] / infos["_final_obs"], single_* and batched spaces."""
    from gym_pybullet_drones_amd.envs import GymVectorEnvAdapter, VectorMultiHoverAviary
    from gym_pybullet_drones_amd.utils.enums import ActionType
    E, D = 32, 2
    base = VectorMultiHoverAviary(E, D, act=ActionType.RPM, ctrl_freq=30, full_obs=True, episode_len_sec=0.2, device=gpu_device)
    venv = GymVectorEnvAdapter(base)
    W = 12 + 15 * 4
    assert venv.num_envs == E and venv.metadata["autoreset_mode"] == "SameStep"
    assert venv.single_observation_space.shape == (D, W) and venv.observation_space.shape == (E, D, W)
    assert venv.single_action_space.shape == (D, 4) and venv.action_space.shape == (E, D, 4)
    obs, infos = venv.reset(seed=1)
    assert obs.shape == (E, D, W) and obs.dtype == np.float32 and infos == {}
    rng = np.random.default_rng(0)
    saw = False
    for k in range(10):
        a = rng.uniform(-1, 1, size=(E, D, 4)).astype(np.float32)
        prev = obs
        obs, rew, term, trunc, infos = venv.step(a)
        assert obs.shape == (E, D, W) and rew.shape == (E,) and term.dtype == bool and trunc.dtype == bool
        np.testing.assert_array_equal(obs[..., -4:], a)
        if (term | trunc).any():
            saw = True
            m = infos["_final_obs"]
            np.testing.assert_array_equal(m, term | trunc)
            assert infos["final_obs"].shape == obs.shape
            # the returned row is the first observation of the new episode, the final one is the finished episode's last
            np.testing.assert_allclose(obs[m][..., 2], 0.1125, atol=1e-6)
            assert (np.abs(infos["final_obs"][m][..., 2] - 0.1125) > 1e-6).any()
            assert not infos["final_obs"][~m].any()
        else:
            assert infos == {}
    assert saw                                   # 0.2 s episodes at 30 Hz: time truncation on step 8
    assert venv.last[0].is_cuda
    venv.close()
    assert venv.closed


def test_lazy_history_is_a_view_and_survives_graph_replay(gpu_device):
    """`full_obs="lazy"`: the step kernel pushes the action into the device ring itself, `history()` is a zero-copy strided
    view of it, `full_rows()` materialises the reference's rows on request -- identical to the eagerly materialised rows
    (`full_obs=True`); and because the ring position lives on the device, a captured hipGraph of steps can be replayed any
    number of times (here across the wrap of the 15-deep ring)."""
    from gym_pybullet_drones_amd.envs import VectorHoverAviary
    from gym_pybullet_drones_amd.utils.enums import ActionType
    E, H, A = 300, 15, 4
    mk = lambda mode: VectorHoverAviary(E, act=ActionType.RPM, ctrl_freq=30, full_obs=mode, auto_reset=True,  # noqa: E731
                                        episode_len_sec=0.3, device=gpu_device)
    eager, lazy, graphed = mk(True), mk("lazy"), mk("lazy")
    rng = np.random.default_rng(4)
    acts = torch.as_tensor(rng.uniform(-1, 1, size=(5, E, 1, A)).astype(np.float32), device=gpu_device)
    for k in range(7):
        o_e, *_ = eager.step(acts[k % 5])
        o_l, *_ = lazy.step(acts[k % 5])
        assert o_l.shape == (E, 1, 12) and o_e.shape == (E, 1, 12 + H * A)
        assert torch.equal(o_e[..., :12], o_l)
    hist = lazy.history()
    assert hist.shape == (E, 1, H, A) and hist.data_ptr() >= lazy.core.act_ring.data_ptr() and not hist.is_contiguous()
    assert hist.untyped_storage().data_ptr() == lazy.core.act_ring.untyped_storage().data_ptr()      # a view, not a copy
    assert torch.equal(hist.reshape(E, 1, H * A), o_e[..., 12:])
    assert torch.equal(lazy.full_rows(), o_e)
    # 3 replays of a 5-step graph after 2 eager steps == 17 eager steps (the ring wraps at 15)
    for k in range(2):
        graphed.step(acts[k])
    torch.cuda.synchronize()
    stream = torch.cuda.Stream(gpu_device)
    stream.wait_stream(torch.cuda.current_stream(gpu_device))
    with torch.cuda.stream(stream):
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, stream=stream):
            for k in range(5):
                graphed.step(acts[(2 + k) % 5])
    torch.cuda.current_stream(gpu_device).wait_stream(stream)
    for _ in range(3):
        g.replay()
    for k in range(7, 17):
        o_e, *_ = eager.step(acts[k % 5])
    torch.cuda.synchronize()
    assert torch.equal(graphed.full_rows(), o_e)
    assert int(graphed.core.ring_pos[0]) == 17 % H and torch.equal(graphed.core.ring_pos, eager.core.ring_pos)
    # rollouts keep the same ring: 6 more steps as one launch on the lazy env, singly on the eager one
    lazy_acts = torch.stack([acts[k % 5] for k in range(7, 13)])
    lazy.rollout(lazy_acts)
    e2 = mk(True)
    for k in range(13):
        o2, *_ = e2.step(acts[k % 5])
    assert torch.equal(lazy.full_rows(), o2)


def test_default_physics_warns_and_rests_on_the_ground(gpu_device):
    """`HoverAviary()` with the reference's defaults asks for Physics.PYB: the explicit integrator runs instead -- said once,
    as a warning -- with the ground plane on, so a drone that does not fly ends up ON the plane (z = COLLISION_H/2), not
    falling through it, and the observation stays inside the advertised observation_space (z >= 0).  Physics.DYN keeps the
    reference's DYN behaviour: no plane."""
    import warnings
    from gym_pybullet_drones_amd.envs import HoverAviary
    from gym_pybullet_drones_amd.utils import enums
    from gym_pybullet_drones_amd.utils.enums import ActionType, Physics
    enums._warned_pyb = False
    with pytest.warns(UserWarning, match="explicit Physics.DYN integrator"):
        env = HoverAviary(act=ActionType.ONE_D_RPM, device=gpu_device)
    with warnings.catch_warnings():
        warnings.simplefilter("error")          # ... once per process
        HoverAviary(act=ActionType.ONE_D_RPM, device=gpu_device)
    obs, _ = env.reset()
    for _ in range(40):                          # 95 % of the hover RPM: sinks 0.1 m in ~0.45 s (30 Hz control)
        obs, rew, term, trunc, _ = env.step(np.array([[-1.0]], dtype=np.float32))
    assert env.pos[0, 2] == pytest.approx(env.COLLISION_H / 2 - env.COLLISION_Z_OFFSET, abs=1e-7)
    assert np.all(env.vel[0] == 0) and env.observation_space.contains(obs)
    dyn = HoverAviary(physics=Physics.DYN, act=ActionType.ONE_D_RPM, device=gpu_device)
    dyn.reset()
    for _ in range(40):
        dyn.step(np.array([[-1.0]], dtype=np.float32))
    assert dyn.pos[0, 2] < 0                     # the reference's DYN: nothing holds the drone


def test_default_physics_in_free_flight_is_the_reference_dyn_bit_for_bit(gpu_device):
    """Round 5 (VERDICT r04 "next" #6): Bullet's damping -- restated from the Bullet sources, pinned against nothing -- is OPT-IN.  The
    drop-in constructors' default `Physics.PYB` is the explicit integrator + the ground plane: above the plane, `HoverAviary()` IS
    `HoverAviary(physics=Physics.DYN)`, observation for observation, bit for bit (the reference side: envs/BaseAviary.py:488-494 loads
    the drone as a Bullet multibody; its own DYN integrator, :831-877, has no damping).  `pyb_like="damped"` / `GPD_PYB_LIKE=damped` /
    `set_pyb_like("damped")` turn the damping on: the same flight then differs."""
    from gym_pybullet_drones_amd.envs import HoverAviary, VectorHoverAviary
    from gym_pybullet_drones_amd.utils import enums
    from gym_pybullet_drones_amd.utils.enums import ActionType, Physics
    assert Physics.PYB.mask() == 8, "the process default must be the ground plane only (GPD_PYB_LIKE unset)"
    pyb, dyn = HoverAviary(act=ActionType.RPM, device=gpu_device), HoverAviary(physics=Physics.DYN, act=ActionType.RPM, device=gpu_device)
    assert pyb._core.physics_flags == 8 and dyn._core.physics_flags == 0
    keep = enums._pyb_like
    try:
        enums.set_pyb_like("damped")
        damped = HoverAviary(act=ActionType.RPM, device=gpu_device)
    finally:
        enums.set_pyb_like(keep)
    assert damped._core.physics_flags == 24
    rng = np.random.default_rng(5)
    o1, _ = pyb.reset(seed=0)
    o2, _ = dyn.reset(seed=0)
    o3, _ = damped.reset(seed=0)
    differs = False
    for k in range(60):                          # 2 s at 30 Hz: climbing (+2.5 % RPM) and drifting a little, never near the plane
        a = (0.5 + 0.03 * rng.uniform(-1, 1, size=(1, 4))).astype(np.float32)
        o1, r1, te1, tr1, _ = pyb.step(a)
        o2, r2, te2, tr2, _ = dyn.step(a)
        o3, *_ = damped.step(a)
        assert np.array_equal(o1, o2) and r1 == r2 and (te1, tr1) == (te2, tr2), k
        differs = differs or not np.array_equal(o1, o3)
    assert pyb.pos[0, 2] > 0.5 and differs
    # the batched classes take the same switch per instance
    v = VectorHoverAviary(4, physics=Physics.PYB, pyb_like="damped", device=gpu_device)
    assert v.core.physics_flags == 24 and VectorHoverAviary(4, physics=Physics.PYB, device=gpu_device).core.physics_flags == 8


def test_subclass_overriding_preprocess_action_with_a_pid_action_type(gpu_device):
    """The reference's subclassing pattern: override `_preprocessAction`, call the base class's mapping, post-process the
    RPMs.  With a PID action type the base mapping runs the embedded DSLPID controllers on the host-side path (`gpd_pid`),
    which needs their state although the step kernel is fed RPMs (round-1 advisor finding: it used to raise GpdError)."""
    from gym_pybullet_drones_amd.envs import HoverAviary
    from gym_pybullet_drones_amd.utils.enums import ActionType, Physics

    class Damped(HoverAviary):
        def _preprocessAction(self, action):
            rpm = super()._preprocessAction(action)
            return np.minimum(rpm, 1.02 * self.HOVER_RPM)          # e.g. a thrust limiter

    plain = HoverAviary(physics=Physics.DYN, act=ActionType.PID, ctrl_freq=240, device=gpu_device)
    sub = Damped(physics=Physics.DYN, act=ActionType.PID, ctrl_freq=240, device=gpu_device)
    assert sub._core.pid is not None and not sub._fused_action and plain._fused_action
    plain.reset(); sub.reset()
    wp = np.array([[0.0, 0.0, 0.12]])
    for k in range(30):
        o1, *_ = plain.step(wp)
        o2, *_ = sub.step(wp)
        assert o2.shape == o1.shape
    # a waypoint 7 mm above the start: the limiter never engages, both envs must follow the same trajectory (fp32 vs the
    # host-side float64 waypoint arithmetic: rounding-level differences only)
    np.testing.assert_allclose(o2[:, :12], o1[:, :12], rtol=0, atol=2e-5)
    assert np.isfinite(sub.last_clipped_action).all() and (sub.last_clipped_action <= 1.02 * sub.HOVER_RPM + 1e-3).all()


def test_logger_export_of_device_states(gpu_device, tmp_path):
    """Logger.log_batch on (N,20) state vectors from the device == N x Logger.log on the rows; CSV/npz files load."""
    from gym_pybullet_drones_amd.envs import VectorCtrlAviary
    from gym_pybullet_drones_amd.utils.Logger import Logger
    n, T = 3, 10
    env = VectorCtrlAviary(1, n, ctrl_freq=48, device=gpu_device)
    a, b = Logger(48, output_folder=str(tmp_path / "a"), num_drones=n), Logger(48, output_folder=str(tmp_path / "b"), num_drones=n)
    rpm = torch.full((1, n, 4), float(env.HOVER_RPM) * 1.02, device=gpu_device)
    for k in range(T):
        env.step(rpm)
        sv = env.state_vectors().view(n, 20)
        a.log_batch(k / 48, sv)
        rows = sv.cpu().numpy()
        for j in range(n):
            b.log(j, k / 48, rows[j])
    a.trim()
    np.testing.assert_array_equal(a.states, b.states)
    np.testing.assert_array_equal(a.timestamps, b.timestamps)
    assert a.states.shape == (n, 16, T) and np.all(a.states[:, 12:16, -1] > 14000)       # rpm columns
    assert np.all(np.diff(a.states[:, 2, :], axis=1) > 0)                                   # climbing
    d = a.save_as_csv("t")
    z = np.loadtxt(d + "/z0.csv", delimiter=",")
    assert z.shape == (T, 2) and z[-1, 1] == pytest.approx(a.states[0, 2, -1])
    a.save()


@pytest.mark.parametrize("N,act", [(1500, "raw_rpm"), (700, "pid")])
def test_swarm_aviary_global_downwash(gpu_device, N, act):
    """ONE aviary of N > 256 drones: gpd_downwash_global (grid binning) + the single-drone step kernel against the
    float64 oracle's O(N^2) loop (envs/BaseAviary.py:785-811).  Drones spread over 60 m x 40 m in 0.3 m layers so that
    many pairs sit inside the 10 m cut-off, several grid cells are populated and dz stays away from the model's
    singularities (dz -> 0+, dz = 0.6875 m) for the pairs that matter."""
    from conftest import urdf
    from gym_pybullet_drones_amd.envs import SwarmAviary
    from gym_pybullet_drones_amd.utils.enums import ActionType, Physics
    from oracle.batched_oracle import BatchedAviary
    rng = np.random.default_rng(N)
    # 12 layers 1 m apart; inside a layer a 4 m lattice with +-0.3 m jitter (same-layer drones stay >= 3 m apart: the
    # model's alpha ~ 1/dz^2 is singular for dz -> 0+), the lattices of the layers aligned so that drones DO fly in each
    # other's wake (dxy <= 0.85 m for vertical neighbours)
    sites = np.array([(x, y) for x in np.arange(-28, 29, 4.0) for y in np.arange(-18, 19, 4.0)])     # 15 x 10
    idx = rng.permutation(len(sites) * 12)[:N]
    layer, site = idx // len(sites), idx % len(sites)
    xyz = np.concatenate([sites[site] + rng.uniform(-0.3, 0.3, size=(N, 2)), (1.0 + 1.0 * layer)[:, None]], axis=1)
    rpy = rng.uniform(-0.05, 0.05, size=(N, 3))
    S = 2
    env = SwarmAviary(N, initial_xyzs=xyz, initial_rpys=rpy, physics=Physics.PYB_GND_DRAG_DW, pyb_freq=240, ctrl_freq=120,
                      act="raw_rpm" if act == "raw_rpm" else ActionType.PID, device=gpu_device)
    orc = BatchedAviary(urdf("cf2x"), "cf2x", num_envs=1, num_drones=N, initial_xyzs=xyz[None], initial_rpys=rpy[None],
                        physics_flags=Physics.PYB_GND_DRAG_DW.mask(True), pyb_freq=240, ctrl_freq=120, act="raw_rpm" if act == "raw_rpm" else "pid", task="none",
                        pid_urdf_path=urdf("cf2x"))
    assert env.nx * env.ny >= 12
    # the force itself, on the initial snapshot
    f = env.downwash().cpu().numpy().astype(np.float64)
    ref = orc.downwash_force_all()[0]
    # exp(-(dxy/beta)^2/2) with |beta| = 0.05 m for the nearest layer has a relative condition number of (dxy/beta)^2 ~ 30
    # against coordinates that fp32 holds to 2e-6 m at |x| ~ 30 m: 3e-3 relative on the individual forces
    np.testing.assert_allclose(f, ref, rtol=3e-3, atol=1e-7)
    assert (np.abs(ref) > 1e-4).mean() > 0.3                # the scene does exercise the term
    for k in range(6):
        if act == "raw_rpm":
            a = (env.HOVER_RPM * (1 + 0.05 * rng.uniform(-1, 1, size=(N, 4)))).astype(np.float32)
            oa = a.astype(np.float64)[None]
        else:
            a = (xyz + rng.uniform(-0.2, 0.2, size=(N, 3))).astype(np.float32)
            oa = a.astype(np.float64)[None]
        sv, *_ = env.step(torch.as_tensor(a, device=gpu_device))
        orc.step(oa)
        got = sv.cpu().numpy().astype(np.float64)
        want = orc.state20()[0]
        scale = np.maximum(np.abs(want).max(axis=0), 1.0)
        err = np.abs(got[:, :16] - want[:, :16]) / scale[:16]
        assert err.max() < (3e-4 if act == "raw_rpm" else 1e-3), (k, err.max(axis=0))
    assert env.step_counter == 6 * S


def test_swarm_downwash_is_order_independent_and_matches_the_workgroup_path(gpu_device):
    """(1) permuting the drones permutes the forces, bit for bit (fixed-point accumulation); (2) for an aviary small
    enough for the fused kernel (D = 200) the global path and the in-kernel LDS path agree."""
    from gym_pybullet_drones_amd.envs import SwarmAviary, VectorCtrlAviary
    from gym_pybullet_drones_amd.utils.enums import Physics
    rng = np.random.default_rng(4)
    N = 200
    xyz = np.stack([rng.uniform(-8, 8, N), rng.uniform(-8, 8, N), 1.0 + 0.3 * rng.integers(0, 10, N) + rng.uniform(-0.01, 0.01, N)], 1)
    perm = rng.permutation(N)
    a = SwarmAviary(N, initial_xyzs=xyz, physics=Physics.PYB_DW, device=gpu_device)
    b = SwarmAviary(N, initial_xyzs=xyz[perm], physics=Physics.PYB_DW, world_min=(-30, -30), world_max=(30, 30), device=gpu_device)
    fa, fb = a.downwash().clone(), b.downwash().clone()
    # (3) the height bins inside a cell only prune candidates that are below every drone of a group: no bins (the default),
    # sixteen 1 m bins, sixty-four 0.25 m bins and five 0.4 m bins (drones in the clamped bottom and top bins) give the same forces, bit for bit
    for kw in (dict(zbin=1.0, nz=16), dict(zbin=0.25, nz=64), dict(zbin=0.4, nz=5)):
        c = SwarmAviary(N, initial_xyzs=xyz, physics=Physics.PYB_DW, device=gpu_device, **kw)
        assert c.nz == kw["nz"] and torch.equal(c.downwash(), fa), kw
        assert torch.equal(c.downwash(), fa)                 # ... also on the second call (visit order = the previous call's order)
    assert torch.equal(fa[torch.as_tensor(perm, device=gpu_device)], fb)
    # (4) more sort keys than the scatter kernel scans in LDS itself (4096): the path with a scan kernel of its own
    big = SwarmAviary(N, initial_xyzs=xyz, physics=Physics.PYB_DW, world_min=(-350, -350), world_max=(350, 350), device=gpu_device)
    assert big.nx * big.ny * big.nz > 4096 and torch.equal(big.downwash(), fa) and torch.equal(big.downwash(), fa)
    # the first call visits the drones as 0, 1, 2 ..., every later one in the previous call's cell order (one atomic per run
    # of equal cells): same forces, and `order` stays a permutation
    for _ in range(3):
        assert torch.equal(a.downwash(), fa)
        # (the rows of the packed position array: the N drones + the rank's meta row)
        assert torch.equal(torch.sort(a._order.long()).values, torch.arange(N + 1, device=gpu_device))
    assert torch.equal(a.downwash_oneshot(), fa)              # ... and the C-ABI's one-call entry, gpd_downwash_global
    v = VectorCtrlAviary(1, N, initial_xyzs=xyz, physics=Physics.PYB_DW, ctrl_freq=240, device=gpu_device)
    rpm = torch.full((N, 4), float(a.HOVER_RPM), device=gpu_device)
    for _ in range(5):
        sa, *_ = a.step(rpm)
        v.step(rpm.view(1, N, 4))
    sv = v.state_vectors().view(N, 20)
    assert torch.allclose(sa, sv, rtol=0, atol=2e-6)


def test_swarm_step_computes_the_next_forces_and_notices_outside_changes(gpu_device):
    """SwarmAviary.step() computes the downwash forces of the NEXT sub-step right after each sub-step (the binning pass also
    writes the state vectors it returns).  Same trajectory, bit for bit, as computing them at the start of each sub-step --
    which is what happens after `core.set_state()` / `invalidate()` / `reset()`; the returned vectors are those of
    `state_vectors()`."""
    from gym_pybullet_drones_amd.envs import SwarmAviary
    from gym_pybullet_drones_amd.utils.enums import Physics
    rng = np.random.default_rng(8)
    N = 700
    xyz = np.stack([rng.uniform(-12, 12, N), rng.uniform(-12, 12, N), 1.0 + 0.5 * rng.integers(0, 8, N) + rng.uniform(-0.01, 0.01, N)], 1)
    a, b = (SwarmAviary(N, initial_xyzs=xyz, physics=Physics.PYB_GND_DRAG_DW, pyb_freq=240, ctrl_freq=120, device=gpu_device) for _ in range(2))
    rpm = torch.as_tensor(a.HOVER_RPM * (1 + 0.01 * rng.uniform(-1, 1, size=(N, 4))).astype(np.float32), device=gpu_device)
    a.reset(); b.reset()
    for k in range(6):
        va, *_ = a.step(rpm)
        if k % 2 == 0:
            b.core.set_state(kin=b.core.kin[:, :N].clone())      # same values: only tells the aviary that its forces are stale
        else:
            b.invalidate()
        vb, *_ = b.step(rpm)
        assert torch.equal(va, vb) and torch.equal(a.core.kin, b.core.kin), k
        assert torch.equal(va, a.state_vectors())
    assert float(a.dw_force.abs().max()) > 1e-4


def test_swarm_downwash_dense_cells_many_tiles_and_large_terms(gpu_device):
    """What the sparse scenes do not reach in the force kernel: a cell with thousands of drones (a group's candidates fill
    several 1024-candidate tiles; nearly every candidate of a chunk passes the test for nearly every lane, so the pair queue
    takes its worst case, 64 x 32 pairs per chunk), and contributions of 4 N and more (two drones 5 cm above each other:
    the 64-bit conversion path).  Against the float64 all-pairs loop of the oracle."""
    from conftest import urdf
    from gym_pybullet_drones_amd.envs import SwarmAviary
    from gym_pybullet_drones_amd.utils.enums import Physics
    from oracle.batched_oracle import BatchedAviary
    rng = np.random.default_rng(21)
    N = 3000
    # thirty layers 0.3 m apart over a 9 m x 9 m patch (one or two grid cells): inside a layer a 0.9 m lattice, the lattices
    # of the layers shifted against each other so that vertical neighbours are >= 0.25 m apart laterally (dz = 0.3 m: |beta| =
    # 0.062 m, the term is ~1e-4 N there and steep), every pair within the 10 m cut-off
    sites = np.array([(x, y) for x in np.arange(0, 9, 0.9) for y in np.arange(0, 9, 0.9)])            # 100
    layer, site = np.divmod(np.arange(N), len(sites))
    xyz = np.concatenate([sites[site] + 0.3 * np.stack([layer % 3, (layer // 3) % 3], 1) + rng.uniform(-0.02, 0.02, size=(N, 2)),
                          (1.0 + 0.3 * layer)[:, None]], axis=1)
    xyz[1] = xyz[0] + np.array([0.001, 0.0, 0.05])          # 0.0762 / 0.05^2 = 30 N on drone 0
    xyz = xyz[rng.permutation(N)]
    env = SwarmAviary(N, initial_xyzs=xyz, physics=Physics.PYB_DW, device=gpu_device)
    orc = BatchedAviary(urdf("cf2x"), "cf2x", num_envs=1, num_drones=N, initial_xyzs=xyz[None], physics_flags=4,
                        pyb_freq=240, ctrl_freq=240, act="raw_rpm", task="none", pid_urdf_path=urdf("cf2x"))
    f = env.downwash().cpu().numpy().astype(np.float64)
    ref = orc.downwash_force_all()[0]
    assert np.abs(ref).max() > 4.0 and (np.abs(ref) > 1e-4).mean() > 0.5
    np.testing.assert_allclose(f, ref, rtol=3e-3, atol=1e-7)
    assert torch.equal(env.downwash(), env.downwash())       # (and again with the previous call's visit order)


def test_swarm_downwash_outside_the_grid_box(gpu_device):
    """The grid is periodic: drones far outside the box it was laid over (and far-apart drones aliasing into
    neighbouring cells) still get exactly the forces of the all-pairs loop."""
    from conftest import urdf
    from gym_pybullet_drones_amd.envs import SwarmAviary
    from gym_pybullet_drones_amd.utils.enums import Physics
    from oracle.batched_oracle import BatchedAviary
    rng = np.random.default_rng(12)
    N = 600
    # three clusters 35 m apart = exactly the period of a 35 m (= 3.5 cells... rounded up to 4 x 10 m) grid laid over the
    # first one, each a small two-layer lattice
    base = np.array([(x, y, 1.0 + l) for l in range(2) for x in np.arange(0, 10, 1.0) for y in np.arange(0, 10, 1.0)])   # 200
    xyz = np.concatenate([base + np.array([ox, oy, 0]) for ox, oy in ((0, 0), (40, 0), (-80, 120))])
    xyz[:, :2] += rng.uniform(-0.2, 0.2, size=(N, 2))
    env = SwarmAviary(N, initial_xyzs=xyz, physics=Physics.PYB_DW, world_min=(-5, -5), world_max=(15, 15), device=gpu_device)
    assert (env.nx, env.ny) == (3, 3)
    orc = BatchedAviary(urdf("cf2x"), "cf2x", num_envs=1, num_drones=N, initial_xyzs=xyz[None], physics_flags=4,
                        pyb_freq=240, ctrl_freq=240, act="raw_rpm", task="none", pid_urdf_path=urdf("cf2x"))
    f = env.downwash().cpu().numpy().astype(np.float64)
    ref = orc.downwash_force_all()[0]
    np.testing.assert_allclose(f, ref, rtol=3e-3, atol=1e-7)
    assert (np.abs(ref) > 1e-4).mean() > 0.1                # (only the lower layer feels a wake, and only under a close neighbour)


def _layered_scene(rng, N, jitter=0.3):
    """12 layers 1 m apart, a 4 m lattice per layer with jitter, the lattices aligned (drones DO fly in each other's wake)"""
    sites = np.array([(x, y) for x in np.arange(-28, 29, 4.0) for y in np.arange(-18, 19, 4.0)])     # 15 x 10
    idx = rng.permutation(len(sites) * 12)[:N]
    layer, site = idx // len(sites), idx % len(sites)
    xyz = np.concatenate([sites[site] + rng.uniform(-jitter, jitter, size=(N, 2)), (1.0 + 1.0 * layer)[:, None]], axis=1)
    return xyz, rng.uniform(-0.05, 0.05, size=(N, 3))


@pytest.mark.parametrize("W,partition", [(2, "spatial"), (3, "index"), (8, "spatial"), (8, "index")])
def test_one_world_shared_by_several_ranks_is_bitwise_the_single_rank_world(gpu_device, W, partition):
    """ONE world sharded across ranks.  Rank r owns a block of drones, steps them, the ranks
    all-gather their positions (here: the in-process exchange of `LocalSwarmGroup`, W ranks on one device), every rank bins
    all positions and evaluates the downwash of its own drones.  The force sums are 64-bit fixed point, hence the demand:
    the sharded world follows the single-rank trajectory BIT FOR BIT -- state vectors and forces, every step, with every
    add-on term and the ground plane on, blocks of unequal size (N not a multiple of W), two sub-steps per control step,
    and different re-binning schedules on the two sides."""
    from gym_pybullet_drones_amd.envs import LocalSwarmGroup, SwarmAviary, swarm_partition
    from gym_pybullet_drones_amd.utils.enums import Physics
    rng = np.random.default_rng(100 + W)
    N = 1501
    xyz, rpy = _layered_scene(rng, N)
    kw = dict(initial_xyzs=xyz, initial_rpys=rpy, physics=Physics.PYB_GND_DRAG_DW, pyb_freq=240, ctrl_freq=120, device=gpu_device)
    one = SwarmAviary(N, rebin_every=1, **kw)
    grp = LocalSwarmGroup(N, W, rebin_every=5, partition=partition, **kw)
    per, slab, counts = swarm_partition(N, W)
    ids = np.concatenate([e.GLOBAL_IDS for e in grp.ranks])
    assert sorted(ids.tolist()) == list(range(N))                        # every drone has exactly one owner
    if partition == "index":
        assert np.array_equal(ids, np.arange(N))
    else:       # stripes: a rank's drones sit in few rows of cells; the groups of 64 sorted drones that hold one of them are ~1/W of all
        rows = [np.unique(np.floor((xyz[e.GLOBAL_IDS, 1] - xyz[:, 1].min()) / 10.5)).size for e in grp.ranks]
        assert max(rows) <= -(-6 // W) + 2, rows
    assert [e.NUM_DRONES for e in grp.ranks] == counts and sum(counts) == N and len(set(counts)) > 1
    v1, _ = one.reset()
    vw = grp.reset()
    assert torch.equal(v1, vw) and torch.equal(one.dw_force[:N], grp.forces())
    assert float(one.dw_force[:N].abs().max()) > 1e-3
    for k in range(12):
        rpm = torch.as_tensor((one.HOVER_RPM * (1 + 0.05 * rng.uniform(-1, 1, size=(N, 4)))).astype(np.float32), device=gpu_device)
        v1, *_ = one.step(rpm)
        vw = grp.step(rpm)
        assert torch.equal(v1, vw), k
        assert torch.equal(one.dw_force[:N], grp.forces()), k
    # every rank holds every drone's position after the exchange, and only its own drones' forces
    for e in grp.ranks:
        assert torch.equal(e.pos4[:, :3].isfinite().all(dim=1).sum(), torch.tensor(N, device=gpu_device))


def _tall_scene(rng, N, jitter=0.3):
    """a world 40 m x 300 m (stripes in y are real stripes), 12 aligned layers 1 m apart on a 4 m lattice"""
    sites = np.array([(x, y) for x in np.arange(-20, 21, 4.0) for y in np.arange(-150, 151, 4.0)])
    idx = rng.permutation(len(sites) * 12)[:N]
    layer, site = idx // len(sites), idx % len(sites)
    xyz = np.concatenate([sites[site] + rng.uniform(-jitter, jitter, size=(N, 2)), (1.0 + 1.0 * layer)[:, None]], axis=1)
    return xyz, rng.uniform(-0.05, 0.05, size=(N, 3))


@pytest.mark.parametrize("W,rebin", [(2, 5), (3, 1), (8, 5), (8, 16)])
def test_halo_exchange_is_bitwise_the_all_gather_world(gpu_device, W, rebin):
    """the cross-GPU HALO exchange.  The ranks of a shared world hold stripes; instead of every rank
    receiving every position (all-gather, 16 B x every drone per sub-step) a rank receives, from its neighbours only, the drones
    within 10 m + margin of its stripe (`HaloPlan`, re-planned with every binning) and bins just those next to its own.  State
    vectors and forces of every drone, every step: bit for bit those of the single-rank world and of the all-gather world, with
    every add-on term on, unequal blocks, two sub-steps per control step; the halo moves a fraction of the all-gather's bytes."""
    from gym_pybullet_drones_amd.envs import LocalSwarmGroup, SwarmAviary
    from gym_pybullet_drones_amd.utils.enums import Physics
    rng = np.random.default_rng(200 + W)
    N = 3001
    xyz, rpy = _tall_scene(rng, N)
    kw = dict(initial_xyzs=xyz, initial_rpys=rpy, physics=Physics.PYB_GND_DRAG_DW, pyb_freq=240, ctrl_freq=120, device=gpu_device)
    one = SwarmAviary(N, rebin_every=1, **kw)
    halo = LocalSwarmGroup(N, W, rebin_every=rebin, exchange="halo", halo_margin=1.0, **kw)
    full = LocalSwarmGroup(N, W, rebin_every=rebin, **kw)
    v1, _ = one.reset()
    vh, vf = halo.reset(), full.reset()
    assert torch.equal(v1, vh) and torch.equal(v1, vf) and torch.equal(one.dw_force[:N], halo.forces())
    assert float(one.dw_force[:N].abs().max()) > 1e-3
    for k in range(14):
        rpm = torch.as_tensor((one.HOVER_RPM * (1 + 0.05 * rng.uniform(-1, 1, size=(N, 4)))).astype(np.float32), device=gpu_device)
        v1, *_ = one.step(rpm)
        vh, vf = halo.step(rpm), full.step(rpm)
        assert torch.equal(v1, vh), k
        assert torch.equal(v1, vf), k
        assert torch.equal(one.dw_force[:N], halo.forces()), k
    sent, allg = halo.bytes_per_substep, full.bytes_per_substep
    print(f"W={W}: halo sends {max(sent)} B per rank and sub-step (plans made: {halo.plans_made}), the all-gather {allg[0]} B")
    assert halo.plans_made >= 28 // rebin
    if W == 8:      # stripes of ~37 m: a rank's halo is its neighbours' 11 m borders, not the world
        assert max(sent) < 0.45 * allg[0]
        inner = halo.ranks[4]
        held = int(inner.pos4[:, :3].isfinite().all(dim=1).sum())
        assert inner.NUM_DRONES < held < 0.5 * N
        assert [c for s_, c in enumerate(halo.plans[4].recv_cnt) if abs(s_ - 4) > 2] == [0] * 3      # far ranks: meta rows only
    # a drone that outruns the margin between two plans: the next plan refuses to go on
    e = halo.ranks[0]
    kin = e.core.kin[:, :e.NUM_DRONES].clone()
    kin[8, 3] = 400.0                                     # 400 m/s in y: > margin / 2 within one sub-step
    e.core.set_state(kin=kin)
    for r in halo.ranks:
        r.invalidate()
    with pytest.raises(RuntimeError, match="halo exchange"):
        for k in range(2 * rebin + 2):
            halo.step(rpm)


def test_halo_world_runs_a_second_episode_after_reset(gpu_device):
    """`reset()` is a teleport, not a margin violation.  A 3-rank halo world in which every drone drifts
    sideways (y) by more than margin / 2 over an episode -- slowly enough that every plan's own interval holds -- is reset to its
    initial poses and flown again: the second episode is bit for bit the first (and the single-rank world's), no RuntimeError;
    the same through set_state() + invalidate() on a real SwarmAviary rank is covered by the resume tests."""
    from gym_pybullet_drones_amd.envs import LocalSwarmGroup, SwarmAviary
    from gym_pybullet_drones_amd.utils.enums import Physics
    rng = np.random.default_rng(77)
    N, margin = 1500, 1.0
    xyz, rpy = _tall_scene(rng, N)
    kw = dict(initial_xyzs=xyz, initial_rpys=rpy, physics=Physics.PYB_GND_DRAG_DW, pyb_freq=240, ctrl_freq=240, device=gpu_device)
    one = SwarmAviary(N, rebin_every=4, **kw)
    halo = LocalSwarmGroup(N, 3, rebin_every=4, exchange="halo", halo_margin=margin, **kw)
    rpm = torch.full((N, 4), float(one.HOVER_RPM), device=gpu_device)

    def push(envs):        # 6 m/s in y for everybody: 0.1 m per 4-sub-step plan interval (< margin / 2), 0.75 m over 30 steps (> margin / 2)
        for e in envs:
            kin = e.core.kin[:, :e.NUM_DRONES].clone()
            kin[8] = 6.0
            e.core.set_state(kin=kin)
            e.invalidate()

    episodes = []
    for ep in range(2):
        v1, _ = one.reset()
        vh = halo.reset()
        assert torch.equal(v1, vh), ep
        push([one] + halo.ranks)
        y0 = v1[:, 1].clone()
        rows = []
        for k in range(30):
            v1, *_ = one.step(rpm)
            vh = halo.step(rpm)
            assert torch.equal(v1, vh), (ep, k)
            rows.append(vh.clone())
        assert float((v1[:, 1] - y0).abs().min()) > 0.5 * margin      # every drone is further from its reset pose than margin / 2
        episodes.append(torch.stack(rows))
    assert torch.equal(episodes[0], episodes[1])
    assert halo.plans_made >= 2 * 7


@pytest.mark.parametrize("W", [1, 8])
def test_worlds_with_many_meta_rows_take_the_ranks_own_displacement_maximum(gpu_device, W):
    """A world with more than 1024 meta rows (one per 256 drones and rank: here 300 000 drones, 1 172 rows; shared by 8 ranks, 8 x 147):
    `gpd_swarm_step` leaves every rank's largest squared displacement in the rank's first meta row (a second, one-workgroup
    launch) and the force launch reads one value per rank instead of all rows.  The search radius and the validity of the wake
    lists hang on that value: a few drones are sent sideways at 40 m/s, so that between two binnings (one side bins every 12th
    sub-step, its twin every sub-step) the radius must widen to two cells and the lists must be given up -- a maximum that
    came out too small would lose pairs.  Forces and state vectors bitwise the twin's, every step."""
    from gym_pybullet_drones_amd.envs import LocalSwarmGroup, SwarmAviary
    from gym_pybullet_drones_amd.utils.enums import Physics
    rng = np.random.default_rng(31 + W)
    sites = np.array([(x, y) for x in np.arange(-300, 300, 4.0) for y in np.arange(-340, 340, 4.0)])      # 150 x 170
    N = 300000
    idx = rng.permutation(len(sites) * 12)[:N]
    xyz = np.concatenate([sites[idx % len(sites)] + rng.uniform(-0.3, 0.3, size=(N, 2)), (1.0 + idx // len(sites))[:, None]], axis=1)
    kw = dict(initial_xyzs=xyz, physics=Physics.PYB_DW, device=gpu_device, pyb_like=False)
    twin = SwarmAviary(N, rebin_every=1, **kw)
    if W == 1:
        env = SwarmAviary(N, rebin_every=12, **kw)
        assert env.WORLD_SIZE * (env.slab - env.per) > 1024
        ranks = [env]
    else:
        env = LocalSwarmGroup(N, W, rebin_every=12, exchange="halo", halo_margin=6.0, **kw)
        assert W * (env.ranks[0].slab - env.ranks[0].per) > 1024
        ranks = env.ranks
    fast = rng.choice(N, 20, replace=False)
    vel = rng.uniform(-1, 1, size=(20, 2)); vel *= 40.0 / np.linalg.norm(vel, axis=1, keepdims=True)
    a = twin.reset()[0] if W == 1 else twin.reset()[0]
    b = env.reset()[0] if W == 1 else env.reset()
    for e in [twin] + ranks:
        ids = np.asarray(e.GLOBAL_IDS)
        kin = e.core.kin[:, :e.NUM_DRONES].clone()
        pos = {int(g): i for i, g in enumerate(ids)}
        for j, f in enumerate(fast):
            if int(f) in pos:
                kin[7, pos[int(f)]], kin[8, pos[int(f)]] = float(vel[j, 0]), float(vel[j, 1])
        e.core.set_state(kin=kin)
        e.invalidate()
    rpm = torch.full((N, 4), float(twin.HOVER_RPM), device=gpu_device)
    saw_wide = False
    for k in range(14):
        a, *_ = twin.step(rpm)
        b = env.step(rpm)[0] if W == 1 else env.step(rpm)
        assert torch.equal(a, b), k
        fa = twin.dw_force[:N]
        fb = env.dw_force[:N] if W == 1 else env.forces()
        assert torch.equal(fa, fb), k
        r0 = ranks[0]
        first_meta = r0.pos4[r0.RANK * r0.slab + r0.per, 3]
        all_meta = r0.pos4[r0.RANK * r0.slab + r0.per:(r0.RANK + 1) * r0.slab, 3]
        assert float(first_meta) == float(all_meta.max())          # the rank's own maximum sits in its first meta row
        saw_wide |= float(first_meta) ** 0.5 > 0.26                # beyond half the skin: R = 2, no replay
    assert saw_wide and float(twin.dw_force[:N].abs().max()) > 1e-3


def test_a_diverged_drone_does_not_turn_the_sub_steps_into_sweeps(gpu_device):
    """the reference's downwash model diverges as dz -> 0+, so a drone CAN be flung to +-inf.  Its displacement since the
    binning is then infinite; taken as the workgroup's maximum it pushed the search radius beyond every bound and turned every
    group of every rank into an O(N^2) sweep until the next binning.  A non-finite position fails every pair test -- it needs no
    search radius: the tracked maximum ignores it, the other drones keep replaying their lists, and their forces are those of
    the same world without that drone."""
    from gym_pybullet_drones_amd.envs import SwarmAviary
    from gym_pybullet_drones_amd.utils.enums import Physics
    rng = np.random.default_rng(5)
    N = 1200
    xyz, rpy = _layered_scene(rng, N)
    kw = dict(initial_xyzs=xyz, initial_rpys=rpy, physics=Physics.PYB_DW, device=gpu_device, pyb_like=False, rebin_every=8)
    env, ref = SwarmAviary(N, **kw), SwarmAviary(N, **kw)
    rpm = torch.full((N, 4), float(env.HOVER_RPM), device=gpu_device)
    for e in (env, ref):
        e.reset()
        e.step(rpm)
    lost = 17
    for e, where in ((env, float("inf")), (ref, 1.0e6)):       # flung to infinity / merely very far away (finite: a legitimate sweep)
        kin = e.core.kin[:, :N].clone()
        kin[0, lost] = where
        e.core.set_state(kin=kin)
        e.invalidate()
    for k in range(6):
        env.step(rpm)
        ref.step(rpm)
        torch.cuda.synchronize()
        keep = torch.arange(N, device=gpu_device) != lost
        assert torch.equal(env.dw_force[:N][keep], ref.dw_force[:N][keep]), k       # nobody is within 10 m of either
        meta = env.pos4[env.per:env.slab, 3]
        assert bool(torch.isfinite(meta).all()) and float(meta.max()) < 1.0, (k, float(meta.max()))      # the radius stays 1
    assert float(env.dw_force[lost]) == 0.0 and not bool(torch.isfinite(env.core.kin[0, lost]))


def test_stale_cell_order_stays_exact_when_drones_outrun_the_skin(gpu_device):
    """Between two binnings the force kernel searches the STALE cell order with a radius that follows the largest displacement
    since the binning (R = ceil((10 m + 2 dmax) / cell); beyond R = 3 a group sweeps every drone).  Drones given lateral
    velocities of up to 40 m/s (and a few at 600 m/s) cross several 10 m cells within the 30 sub-steps of this test while one
    side never re-bins: forces and trajectories stay those of the side that re-bins before every force evaluation, bit for
    bit -- and those of the float64 all-pairs loop."""
    from conftest import urdf
    from gym_pybullet_drones_amd.envs import SwarmAviary
    from gym_pybullet_drones_amd.utils.enums import Physics
    from oracle import c_oracle
    rng = np.random.default_rng(77)
    N = 1200
    xyz, rpy = _layered_scene(rng, N)
    kw = dict(initial_xyzs=xyz, initial_rpys=rpy, physics=Physics.PYB_DW, device=gpu_device, pyb_like=False, cell=10.0)
    fresh, stale = SwarmAviary(N, rebin_every=1, **kw), SwarmAviary(N, rebin_every=10 ** 6, **kw)
    vel = rng.uniform(-40, 40, size=(N, 2))
    vel[:5] = rng.uniform(-600, 600, size=(5, 2))
    for e in (fresh, stale):
        e.reset()
        kin = e.core.kin[:, :N].clone()
        kin[7:9] = torch.as_tensor(vel.T, dtype=torch.float32, device=gpu_device)
        e.core.set_state(kin=kin)
    rpm = torch.full((N, 4), float(fresh.HOVER_RPM), device=gpu_device)
    for k in range(30):
        a, *_ = fresh.step(rpm)
        b, *_ = stale.step(rpm)
        assert torch.equal(a, b), k
        assert torch.equal(fresh.dw_force, stale.dw_force), k
        if k in (0, 9, 29):
            ref = c_oracle.downwash_all_pairs(urdf("cf2x"), stale.core.kin[0:3, :N].t().cpu().numpy().astype(np.float64))
            np.testing.assert_allclose(stale.dw_force[:N].cpu().numpy().astype(np.float64), ref, rtol=3e-3, atol=1e-7)
    assert stale._since_bin == 30 and fresh._since_bin == 0
    moved = (stale.core.kin[0:2, :N].t().cpu().numpy() - xyz[:, :2])
    assert np.abs(moved).max() > 30.0                       # several cells


@pytest.mark.parametrize("rebin", [3, 16])
def test_swarm_steps_captured_in_a_hipgraph_replay_like_eager_steps(gpu_device, rebin):
    """A captured hipGraph of swarm steps bakes in WHICH sub-steps re-bin; replayed after eager calls that re-binned on a
    schedule of their own (a reset between two replays), it must still follow the eager trajectory bit for bit: `order` is one
    buffer that always belongs to the latest binning, whatever ran in between."""
    from gym_pybullet_drones_amd.envs import SwarmAviary
    from gym_pybullet_drones_amd.utils.enums import Physics
    rng = np.random.default_rng(5)
    N = 900
    xyz, rpy = _layered_scene(rng, N)
    kw = dict(initial_xyzs=xyz, initial_rpys=rpy, physics=Physics.PYB_GND_DRAG_DW, device=gpu_device, rebin_every=rebin)
    a, b = SwarmAviary(N, **kw), SwarmAviary(N, **kw)
    rpm = torch.as_tensor((a.HOVER_RPM * (1 + 0.02 * rng.uniform(-1, 1, size=(20, N, 4)))).astype(np.float32), device=gpu_device)
    for e in (a, b):
        e.reset()
        for k in range(5):
            e.step(rpm[k])
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    stream = torch.cuda.Stream(gpu_device)
    stream.wait_stream(torch.cuda.current_stream(gpu_device))
    with torch.cuda.stream(stream):
        with torch.cuda.graph(g, stream=stream):
            for k in range(20):
                vb, *_ = b.step(rpm[k])
    torch.cuda.current_stream(gpu_device).wait_stream(stream)
    for rep in range(3):
        a.reset(); b.reset()                       # (eager: re-bins, out of step with the schedule the graph has baked in)
        if rep == 2:
            a.step(rpm[0]); b.step(rpm[0])         # ... and an eager step, so that the two sides' host counters differ from capture time
        for k in range(20):
            va, *_ = a.step(rpm[k])
        g.replay()
        torch.cuda.synchronize()
        assert torch.equal(va, vb) and torch.equal(a.core.kin, b.core.kin), rep
        assert torch.equal(a.dw_force, b.dw_force), rep


@pytest.mark.parametrize("adaptive", [True, False], ids=["margin follows the motion", "full margin"])
@pytest.mark.parametrize("variant", ["lists", "overflowing lists", "outrun lists", "in transit", "one fast drone"])
def test_wake_lists_replay_the_pairs_of_the_last_binning_exactly(gpu_device, variant, adaptive):
    """Between two binnings the force launches replay the pairs the launch after the binning evaluated (kept with a margin of
    `list_delta` per drone) instead of sweeping all candidates.  Same forces and trajectories, bit for bit, as a twin that bins
    before every force evaluation (no lists at all) -- also when most groups' lists overflow their capacity (those groups sweep),
    and when drones move further than `list_delta` RELATIVE TO EACH OTHER between two binnings (every group sweeps, with the
    radius of `test_stale_cell_order_stays_exact_when_drones_outrun_the_skin`).  A swarm in transit -- every drone at 6 m/s the
    same way -- keeps its lists: displacement is measured against the swarm's common drift, the tracked residual stays a
    fraction of `list_delta` while every drone has moved several times that.  `adaptive`: every binning picks the margin of its
    lists from the displacement the interval before it saw (1 cm ... `list_delta`), or always `list_delta`: the lists differ,
    the forces do not.  ONE drone crossing the hovering swarm at 3 m/s outruns an adapted margin within a sub-step (every group
    sweeps until the next binning, whose margin then follows that drone up to what the skin allows) -- same bits."""
    from gym_pybullet_drones_amd.envs import SwarmAviary
    from gym_pybullet_drones_amd.utils.enums import Physics
    rng = np.random.default_rng(31)
    N = 1700
    xyz, rpy = _layered_scene(rng, N)
    kw = dict(initial_xyzs=xyz, initial_rpys=rpy, physics=Physics.PYB_GND_DRAG_DW, device=gpu_device, cell=10.5)
    ref = SwarmAviary(N, rebin_every=1, **kw)
    env = SwarmAviary(N, rebin_every=12, list_cap=4 if variant == "overflowing lists" else 48, adaptive_lists=adaptive, **kw)
    assert env.wake_lists and not ref.wake_lists and 0.2 < env.list_delta < 0.25
    for e in (ref, env):
        e.reset()
        if variant in ("outrun lists", "in transit"):      # 6 m/s sideways: 0.245 m -- list_delta -- after ten sub-steps
            kin = e.core.kin[:, :N].clone()
            kin[7] = 6.0
            if variant == "outrun lists":                   # ... half of them the other way
                kin[7, ::2] = -6.0
            e.core.set_state(kin=kin)
        if variant == "one fast drone":                    # 3 m/s: 0.15 m in twelve sub-steps, inside the skin, beyond an adapted margin
            kin = e.core.kin[:, :N].clone()
            kin[7, 5] = 3.0
            e.core.set_state(kin=kin)
    rpm = torch.as_tensor((ref.HOVER_RPM * (1 + 0.02 * rng.uniform(-1, 1, size=(N, 4)))).astype(np.float32), device=gpu_device)
    checked_drift = False
    for k in range(30):
        a, *_ = ref.step(rpm)
        b, *_ = env.step(rpm)
        assert torch.equal(a, b), k
        assert torch.equal(ref.dw_force, env.dw_force), k
        if variant in ("outrun lists", "in transit") and env._since_bin == env.rebin_every - 1:      # (just before a binning)
            true_d2 = float(((env.pos4[:N, :3] - env._bin_pos[:N, :3]) ** 2).sum(dim=1).max())
            tracked = float(env.pos4[N:, 3].max())
            assert true_d2 > env.list_delta ** 2             # (every drone is further from where it was binned than the lists allow)
            assert (tracked < 0.25 * env.list_delta ** 2) == (variant == "in transit"), (tracked, true_d2)
            checked_drift = True
    assert checked_drift == (variant in ("outrun lists", "in transit"))
    margin = float(env._drift[2])                   # what the last binning chose
    if not adaptive or variant == "outrun lists":
        assert margin == np.float32(env.list_delta)
    elif variant == "one fast drone":               # the margin follows the fastest drone
        assert margin > 0.1
    else:                                           # hovering, or all in transit together: centimetres relative to the drift
        assert 0.01 <= margin < 0.5 * env.list_delta, margin
    ok = env._list_ok[:(N + 63) // 64].float().mean().item()
    assert float(ref.dw_force[:N].abs().max()) > 1e-3
    if variant == "lists":
        assert ok == 1.0                            # every group replays
    elif variant == "overflowing lists":
        assert ok < 0.5                             # most groups evaluate more than one batch per wave: they sweep


def test_kinematic_planes_are_writable_views_and_kin_is_their_logical_matrix(gpu_device):
    """ABI 9 on the Python side: `SimCore.kin_P / kin_Q / kin_V / kin_W` are views of the one state buffer the kernels read and write,
    `positions() / quaternions() / velocities()` views of those, `kin` the logical [13][ld] matrix (a copy), `set_state(kin=...)` its
    inverse.  A velocity written through a view is what the next step integrates."""
    from gym_pybullet_drones_amd.envs import VectorHoverAviary
    from gym_pybullet_drones_amd.utils.enums import ActionType, Physics
    env = VectorHoverAviary(64, physics=Physics.DYN, act=ActionType.RPM, ctrl_freq=240, auto_reset=False, device=gpu_device)
    c = env.core
    env.reset()
    k = c.kin
    assert k.shape == (13, c.ld) and torch.equal(k[0:3, :64].t(), c.positions()) and torch.equal(k[3:7, :64].t(), c.quaternions())
    assert torch.equal(k[7:10, :64].t(), c.velocities()) and torch.equal(k[10:13, :64].t(), c.body_rates())
    assert c.kin_P.data_ptr() == c.kin_store.data_ptr() and c.kin_W.data_ptr() == c.kin_store.data_ptr() + 12 * c.ld * 4
    np.testing.assert_allclose(c.positions().cpu().numpy(), np.broadcast_to(c.INIT_XYZS, (64, 1, 3)).reshape(64, 3), atol=1e-7)
    z0 = c.positions()[:, 2].clone()
    c.velocities()[:, 2] = 1.2                                     # written through the view ...
    env.step(torch.zeros((64, 1, 4), device=gpu_device))           # ... hover RPMs: z advances by v dt
    np.testing.assert_allclose((c.positions()[:, 2] - z0).cpu().numpy(), 1.2 / 240, rtol=1e-4)
    with pytest.raises(TypeError, match="copy of the state"):      # (up to ABI 8 this assignment changed the device's state: now it says so)
        c.kin[8, 3] = 1.0
    for lost_write in (lambda: c.kin[0:3].copy_(torch.zeros(3, c.ld, device=gpu_device)), lambda: c.kin[2].fill_(1.0),
                       lambda: c.kin[:, 5].zero_()):         # in-place operations on the copy or on a view of it
        with pytest.raises(TypeError, match="copy of the state"):
            lost_write()
    snap = c.kin[:, :64].clone()
    snap[8] = -0.5
    c.set_state(kin=snap)
    assert torch.equal(c.kin[:, :64], snap) and float(c.kin_V[3, 1]) == -0.5


@pytest.mark.parametrize("act,D,flags,S", [(0, 1, 0, 8), (1, 1, 0, 8), (0, 3, 7, 2), (2, 2, 2, 5)])
def test_host_visible_core_is_bitwise_the_device_core(gpu_device, act, D, flags, S):
    """`SimCore(host_visible=True)` -- what the reference-shaped single aviaries run on since round 6: state, action row and step
    outputs in page-locked host memory the kernel addresses directly -- is the same kernels on the same bits: 60 steps, a masked
    reset and a rollout in lock-step with a core whose state lives in HBM; state, observation rows, rewards, flags, counters and
    the controllers' members equal bit for bit.  And a `step()` of it has drained the stream when it returns (the host reads
    the buffers without a copy)."""
    from gym_pybullet_drones_amd import engine
    rng = np.random.default_rng(act + 10 * D)
    xyz = rng.uniform(-0.3, 0.3, size=(D, 3)) + np.array([0, 0, 0.5]) + np.arange(D)[:, None] * np.array([0.15, 0, 0.3])
    kw = dict(num_envs=1, drones_per_env=D, physics=flags, pyb_freq=240, ctrl_freq=240 // S, act_code=act, task=engine.TASK_HOVER if D == 1 else engine.TASK_MULTIHOVER,
              initial_xyzs=xyz, initial_rpys=rng.uniform(-0.1, 0.1, size=(D, 3)), target_pos=xyz + np.array([0, 0, 0.3]), track_rpm=True,
              nan_guard=True, device=gpu_device)
    hv, dv = engine.SimCore(host_visible=True, **kw), engine.SimCore(**kw)
    assert hv.kin_store.device.type == "cpu" and hv.kin_store.is_pinned() and hv.action_host.is_pinned() and dv.kin_store.device == gpu_device
    A = hv.A

    def same():
        torch.cuda.synchronize()
        for name in ("kin_store", "last_rpm", "pid", "step_counter", "obs12", "reward", "terminated", "truncated", "bad"):
            a, b = getattr(hv, name), getattr(dv, name)
            assert (a is None) == (b is None), name
            if a is not None:
                assert torch.equal(a, b.cpu()), name

    same()
    for k in range(60):
        a = rng.uniform(-1, 1, size=(D, A)).astype(np.float32) * (0.3 if act != 1 else 1.0) + (np.array([0, 0, 0.8], dtype=np.float32) if act == 1 else 0)
        hv.action_host.numpy()[...] = a
        o, r, te, tr = hv.step(hv.action_host)
        # no synchronisation here on purpose: the host-visible step returned after its stream drained
        assert np.isfinite(o.numpy()).all() and o.numpy().shape == (D, 12)
        dv.step(torch.as_tensor(a, device=gpu_device))
        if k % 10 == 9:
            same()
        if k == 30:
            hv.reset(mask=torch.ones(1, dtype=torch.uint8, device=gpu_device))
            dv.reset(mask=torch.ones(1, dtype=torch.uint8, device=gpu_device))
            same()
    acts = torch.as_tensor(rng.uniform(-0.2, 0.2, size=(5, D, A)).astype(np.float32), device=gpu_device)
    oh, rh, _, _ = hv.rollout(acts)
    od, rd, _, _ = dv.rollout(acts)
    assert torch.equal(oh.cpu(), od.cpu()) and torch.equal(rh.cpu(), rd.cpu())
    same()
    st = hv.get_state()
    hv.step(hv.action_host)
    hv.set_state(**st)
    dv.set_state(**{k: v.to(gpu_device) for k, v in st.items()})
    same()


def test_dropin_aviary_step_is_one_launch_on_host_visible_state(gpu_device, monkeypatch):
    """The reference-shaped `HoverAviary.step()`: the action row written where the kernel reads it, ONE library call (gpd_step_sync:
    one launch + the wait for its stream), no gpd_state_vectors launch, no torch.cat / device-to-host copy -- and the same
    trajectory, float for float, as with GPD_HOST_VISIBLE=0 (state in HBM, the round-5 path with its packed copy)."""
    from gym_pybullet_drones_amd import _native
    from gym_pybullet_drones_amd.envs import HoverAviary, MultiHoverAviary
    from gym_pybullet_drones_amd.utils.enums import ActionType, Physics
    rng = np.random.default_rng(4)
    for make, A in ((lambda: HoverAviary(physics=Physics.DYN, act=ActionType.ONE_D_RPM, device=gpu_device), (1, 1)),
                    (lambda: MultiHoverAviary(num_drones=3, physics=Physics.DYN, act=ActionType.PID, device=gpu_device), (3, 3))):
        monkeypatch.setenv("GPD_HOST_VISIBLE", "1")
        a = make()
        monkeypatch.setenv("GPD_HOST_VISIBLE", "0")
        b = make()
        assert a._core.host_visible and not b._core.host_visible
        oa, _ = a.reset(seed=1)
        ob, _ = b.reset(seed=1)
        np.testing.assert_array_equal(oa, ob)
        L = _native.lib()
        calls = {"gpd_step_sync": 0, "gpd_step": 0, "gpd_state_vectors": 0}
        real = {n: getattr(L, n) for n in calls}
        for n in calls:
            def counted(*args, _n=n):
                calls[_n] += 1
                return real[_n](*args)
            monkeypatch.setattr(L, n, counted, raising=False)
        acts = rng.uniform(-1, 1, size=(40,) + A).astype(np.float32) * 0.3 + (np.array([0, 0, 0.7], dtype=np.float32) if A[1] == 3 else 0)
        for k in range(40):
            ra = a.step(acts[k])
            assert calls == {"gpd_step_sync": k + 1, "gpd_step": 0, "gpd_state_vectors": 0}
            n0 = dict(calls)
            rb = b.step(acts[k])
            calls.update(n0)
            np.testing.assert_array_equal(ra[0], rb[0])
            assert ra[1:4] == rb[1:4] and isinstance(ra[1], float) and isinstance(ra[2], bool)
            for name in ("pos", "quat", "rpy", "vel", "ang_v", "rpy_rates", "last_clipped_action"):
                x, y = getattr(a, name), getattr(b, name)
                assert x.dtype == np.float64 and x.shape == y.shape
                np.testing.assert_array_equal(x, y, err_msg=name)
            np.testing.assert_array_equal(a._getDroneStateVector(0), b._getDroneStateVector(0))
        for n in calls:
            monkeypatch.setattr(L, n, real[n], raising=False)
        text = a.render()
        assert text.count("\n") == 1 + a.NUM_DRONES and "sim" in text.split("\n")[0]
        a.close(); b.close()


@pytest.mark.parametrize("D,act,E,lanes", [pytest.param(1, "one_d_rpm", 1, 64, id="1-one_d_rpm"), pytest.param(3, "pid", 1, 64, id="3-pid"),
                                           pytest.param(70, "rpm", 1, 64, id="70-rpm"),
                                           # several single-drone aviaries, (num_envs, lanes_per_wave): all in wave 0 (12 <= 16, 40 <= 64: the
                                           # completion word), or past it (40 > 16, 70 > 32: hipStreamSynchronize)
                                           pytest.param(1, "rpm", 12, 16, id="envs12-lanes16"), pytest.param(1, "rpm", 40, 16, id="envs40-lanes16"),
                                           pytest.param(1, "rpm", 40, 64, id="envs40-lanes64"), pytest.param(1, "rpm", 70, 32, id="envs70-lanes32")])
def test_step_sync_returns_only_when_the_results_are_readable(gpu_device, D, act, E, lanes):
    """`gpd_step_sync` (what `BaseAviary.step()` calls) learns that the step is done from a word the kernel itself writes into
    page-locked memory when the aviary fits one wavefront, and from hipStreamSynchronize otherwise (70 drones: two waves; every 256th
    call; a stream with work queued ahead).  Whatever the way: when it returns, the buffers hold THIS step's results -- 700 steps
    read back at once, each compared bit for bit with a core in HBM that is synchronised the slow way, across the 256-call
    boundary, a reset in between, and once with a large kernel queued ahead on the stream.  With several single-drone aviaries (330
    steps) the word is written only if they all sit in wave 0 of workgroup 0, which `lanes_per_wave` decides with their number."""
    from gym_pybullet_drones_amd import engine
    rng = np.random.default_rng(D if E == 1 else 1000 * E + lanes)
    steps, reset_at, ballast_at = (700, 300, 400) if E == 1 else (330, 280, 300)
    code = {"rpm": 0, "pid": 1, "one_d_rpm": 3}[act]
    xyz = rng.uniform(-0.3, 0.3, size=(D, 3)) * np.array([1, 1, 0]) + np.array([0, 0, 0.5]) + np.arange(D)[:, None] * np.array([0.3, 0.1, 0.0])
    kw = dict(num_envs=E, drones_per_env=D, physics=0, pyb_freq=240, ctrl_freq=30, act_code=code, task=engine.TASK_HOVER if D == 1 else engine.TASK_MULTIHOVER,
              initial_xyzs=xyz, initial_rpys=np.zeros((D, 3)), target_pos=xyz + np.array([0, 0, 0.3]), track_rpm=True, device=gpu_device)
    hv, dv = engine.SimCore(host_visible=True, **kw), engine.SimCore(**kw)
    hv._cfg.lanes_per_wave = dv._cfg.lanes_per_wave = lanes
    obs_h, rew_h, kin_h = hv.obs12.numpy(), hv.reward.numpy(), hv.kin_store.numpy()
    ballast = torch.empty(1 << 28, dtype=torch.float32, device=gpu_device)              # 1 GiB: a fill of it takes ~0.2 ms
    for k in range(steps):
        a = (rng.uniform(-1, 1, size=(E * D, hv.A)) * 0.05).astype(np.float32) + (np.array([0, 0, 0.8], dtype=np.float32) if act == "pid" else 0)
        hv.action_host.numpy()[...] = a
        if k == ballast_at:
            for _ in range(20):
                ballast.fill_(float(k))                                                  # ~4 ms of work ahead of the step on its stream
        hv.step_host()
        got = (obs_h.copy(), rew_h.copy(), kin_h.copy())                                # read at once: no synchronisation of ours
        dv.step(torch.as_tensor(a, device=gpu_device))
        torch.cuda.synchronize()
        assert np.array_equal(got[0], dv.obs12.cpu().numpy()), k
        assert np.array_equal(got[1], dv.reward.cpu().numpy()), k
        assert np.array_equal(got[2], dv.kin_store.cpu().numpy()), k
        if k == reset_at:
            hv.reset()
            dv.reset()
    assert np.isfinite(got[0]).all()
