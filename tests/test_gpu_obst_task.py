"""The obstacle task on the MI355X: one `gpd_rollout_obst` launch against (a) `gpd_rollout` where nothing is near and (b) the composition
of the entries the library already had -- per step `gpd_step` without auto-reset, `gpd_obstacles` for clearance and contact, elementwise
torch for reward and termination, a masked `gpd_reset`, `gpd_obstacles` again for the clearance and the scan of the pose that is
observed -- over the cases of tests/helpers/obst_task_f64.py.  Every comparison is BIT FOR BIT, with no exclusions: rows, rewards,
flags, the final state, counters, last RPMs and controller members; every output sits in a buffer larger than needed whose other
words must keep their sentinel.  Then the class: `reset()` against an auto-reset, `rollout(K)` against K `step()` calls, the adapters,
and a refused call.

MEASURED on an MI355X, on the composed runs of the cases with K = 5 and N >= 70: 30.7-41.4 % of the drones collide (24 to 95 of them
before the last step), 41.3-53.3 % of the rays hit, the hinge of the drones that never collide lies in 0.009 .. 0.486, and up to 37
aviaries are truncated (rpm_shared65_r16_world: its course reaches past the hover task's bounds)."""
import functools
import os
import sys

import numpy as np
import pytest
import torch

from conftest import REPO

sys.path.insert(0, os.path.join(REPO, "tests", "helpers"))
import obst_task_f64 as yo  # noqa: E402

pytestmark = pytest.mark.gpu

IDS = [c.name for c in yo.CASES]
SENT_F, SENT_B = -77.0, 200
TASKS = {"none": 0, "hover": 1}


def bits(t):
    return t.contiguous().view(torch.int32) if t.dtype == torch.float32 else t.contiguous().view(torch.uint8)


def same(a, b):
    return a.shape == b.shape and torch.equal(bits(a), bits(b))


def make_core(case, sc, dev, auto_reset):
    """a core in the scene's start state: tilted, moving, turning, controller members and last RPMs that are not zero, step counters
    of which one is about to run out (hover: a truncation by time inside the flight)"""
    from gym_pybullet_drones_amd import engine
    core = engine.SimCore(num_envs=case.N, drones_per_env=1, physics=case.flags, pyb_freq=yo.PYB_FREQ, ctrl_freq=yo.PYB_FREQ // case.S,
                          act_code=yo.ACT_CODE[case.act], task=TASKS[case.task], initial_xyzs=sc.init_xyz[:, None, :],
                          initial_rpys=sc.init_rpy[:, None, :], target_pos=np.array([[0.0, 0.0, 1.0]]), auto_reset=bool(auto_reset),
                          track_rpm=True, device=dev)
    counters = (np.arange(case.N) % 7) * case.S
    if case.N > 3:
        counters[3] = core._cfg.trunc_counter - 2 * case.S
    core.set_state(kin=sc.kin, pid=sc.pid if core.pid is not None else None, last_rpm=sc.last_rpm, step_counter=counters.astype(np.int32))
    return core


def state_of(core):
    return {"kin": core.kin_store.clone(), "counter": core.step_counter.clone(), "last_rpm": None if core.last_rpm is None else core.last_rpm.clone(),
            "pid": None if core.pid is None else core.pid.clone()}


def same_state(a, b):
    return all((a[k] is None and b[k] is None) or same(a[k], b[k]) for k in a)


def task_of(case, hit_terminates=1):
    from gym_pybullet_drones_amd import _native
    return _native.GpdObstTask(collision_radius=yo.COLLISION_RADIUS, hit_terminates=hit_terminates, hit_reward=yo.HIT_REWARD,
                               prox_margin=yo.PROX_MARGIN, prox_weight=yo.PROX_WEIGHT, n_rays=case.rays, ray_frame=yo.FRAMES[case.frame],
                               max_range=yo.MAX_RANGE)


def fused(case, sc, dev, hit_terminates=1):
    """ONE launch into buffers larger than needed -- a row pitch of 16 + R rounded up plus 4, step strides with slack, sentinels
    everywhere -> dict of the outputs, the final state; asserts that no word outside the outputs was written"""
    from gym_pybullet_drones_amd import _native
    core = make_core(case, sc, dev, case.auto_reset)
    N, K, R = case.N, case.K, case.rays
    W = 16 + R
    row_ld = (W + 3) // 4 * 4 + 4
    row_stride, env_stride = N * row_ld + 8, N + 5
    rows = torch.full((K * row_stride + 16,), SENT_F, dtype=torch.float32, device=dev)
    reward = torch.full((K * env_stride + 3,), SENT_F, dtype=torch.float32, device=dev)
    flags = [torch.full((K * env_stride + 3,), SENT_B, dtype=torch.uint8, device=dev) for _ in range(3)]
    actions = torch.as_tensor(sc.actions, device=dev).contiguous()
    table = torch.as_tensor(sc.table, device=dev).contiguous()
    rays = None if sc.rays is None else torch.as_tensor(sc.rays, device=dev).contiguous()
    _native.call("gpd_rollout_obst", dev, core._stream(), core._params, core._state, core._cfg, task_of(case, hit_terminates), K, actions,
                 N * yo.ACT_DIM[case.act], core.target, core.init_pose, table, sc.n_obst, sc.obst_ld, rays, rows, row_ld, row_stride, reward,
                 flags[0], flags[1], flags[2], env_stride)
    torch.cuda.synchronize()
    block = rows[:K * row_stride].view(K, row_stride)
    rows_v = block[:, :N * row_ld].reshape(K, N, row_ld)
    assert (rows_v[..., W:] == SENT_F).all() and (block[:, N * row_ld:] == SENT_F).all() and (rows[K * row_stride:] == SENT_F).all()
    out = {"rows": rows_v[..., :W].clone()}
    for name, buf, sent in (("reward", reward, SENT_F), ("terminated", flags[0], SENT_B), ("truncated", flags[1], SENT_B), ("collided", flags[2], SENT_B)):
        v = buf[:K * env_stride].view(K, env_stride)
        assert (v[:, N:] == sent).all() and (buf[K * env_stride:] == sent).all(), name
        out[name] = v[:, :N].clone()
    assert all((out[k] <= 1).all() for k in ("terminated", "truncated", "collided"))
    return out, state_of(core)


def composed(case, sc, dev, hit_terminates=1):
    """the five-step recipe, K times, on a core without auto-reset -> the same dict, the final state, and the hinge of every step"""
    from gym_pybullet_drones_amd import _native
    core = make_core(case, sc, dev, False)
    N, K, R, M = case.N, case.K, case.rays, sc.n_obst
    f32 = lambda v: torch.tensor(v, dtype=torch.float32, device=dev)  # noqa: E731
    r, hr, pm, pw = f32(yo.COLLISION_RADIUS), f32(yo.HIT_REWARD), f32(yo.PROX_MARGIN), f32(yo.PROX_WEIGHT)
    actions = torch.as_tensor(sc.actions, device=dev).contiguous()
    table = torch.as_tensor(sc.table, device=dev).contiguous()
    rays = None if sc.rays is None else torch.as_tensor(sc.rays, device=dev).contiguous()
    clear4, hit = torch.zeros((N, 4), device=dev), torch.zeros(N, dtype=torch.uint8, device=dev)
    ranges = torch.zeros((N, max(R, 1)), device=dev)
    out = {"rows": torch.zeros((K, N, 16 + R), device=dev), "reward": torch.zeros((K, N), device=dev)}
    out.update({k: torch.zeros((K, N), dtype=torch.uint8, device=dev) for k in ("terminated", "truncated", "collided")})
    hinges = torch.zeros((K, N), device=dev)

    def query(with_scan):
        _native.call("gpd_obstacles", dev, core._stream(), core.kin_P, core.kin_Q, N, 1, table, M, sc.obst_ld, yo.COLLISION_RADIUS, clear4, None,
                     hit, rays if with_scan else None, R if with_scan else 0, yo.FRAMES[case.frame], yo.MAX_RANGE if with_scan else 0.0,
                     ranges if with_scan else None, None)

    for t in range(K):
        _, rew, term, trunc = core.step(actions[t])                         # 1. the step, no auto-reset
        query(False)                                                        # 2. clearance and contact of the pose it reached
        d, hitb = clear4[:, 3], hit.bool()
        hinge = torch.clamp_min(pm - (d - r), 0.0)                          # 3. reward and termination
        rew2 = torch.where(hitb, rew + hr, rew) - pw * hinge
        term2 = term | hitb if hit_terminates else term.clone()
        if case.auto_reset:
            core.reset(mask=term2 | trunc)                                  # 4. the masked reset
        query(R > 0)                                                        # 5. clearance and scan of the pose that is observed
        out["rows"][t, :, :12] = core.obs12
        out["rows"][t, :, 12:16] = clear4
        if R:
            out["rows"][t, :, 16:] = ranges
        out["reward"][t], out["terminated"][t], out["truncated"][t], out["collided"][t] = rew2, term2, trunc, hitb
        hinges[t] = hinge
    torch.cuda.synchronize()
    return out, state_of(core), hinges


@functools.lru_cache(maxsize=None)
def flown(name, hit_terminates=1):
    """one case flown both ways, once per session (the tests below share it and leave it unchanged)"""
    case = next(c for c in yo.CASES if c.name == name)
    dev = torch.device("cuda", torch.cuda.current_device())
    sc = yo.scene(case)
    return case, sc, fused(case, sc, dev, hit_terminates), composed(case, sc, dev, hit_terminates)


@pytest.mark.parametrize("name", IDS)
def test_one_launch_is_the_composition_of_the_existing_entries_bit_for_bit(gpu_device, name):
    case, sc, (got, got_state), (want, want_state, _) = flown(name)
    for k in ("collided", "terminated", "truncated", "reward", "rows"):
        if not same(got[k], want[k]):
            bad = (bits(got[k]) != bits(want[k])).nonzero()
            pytest.fail(f"{name}: {k} differs at {len(bad)} places, first {bad[0].tolist()}: {got[k][tuple(bad[0])].item()} vs {want[k][tuple(bad[0])].item()}")
    assert same_state(got_state, want_state), name


@pytest.mark.parametrize("name", [c.name for c in yo.CASES if c.K == 5 and c.N >= 70])
def test_scene_exercises_what_it_claims(gpu_device, name):
    """on the COMPOSED run: 25-45 % of the drones collide, some of them before the last step (steps after a reset are compared), at least
    20 % of the rays hit, the proximity term is non-zero for drones that never collide, and the reset pose inside an obstacle collides at
    every step after its aviary's first reset"""
    case, sc, _, (want, _, hinges) = flown(name)
    coll = want["collided"].bool()
    share, early = float(coll.any(dim=0).float().mean()), int(coll[:case.K - 1].any(dim=0).sum())
    rays_hit = float((want["rows"][..., 16:] < yo.MAX_RANGE).float().mean()) if case.rays else None
    clear = ~coll.any(dim=0)
    print(f"{name}: collided {share:.3f} (before the last step: {early} drones), rays that hit {rays_hit}, "
          f"hinge of the others {float(hinges[:, clear].min()):.3f} .. {float(hinges[:, clear].max()):.3f}, truncated {int(want['truncated'].sum())}")
    assert 0.25 <= share <= 0.45 and early > 0
    assert rays_hit is None or rays_hit >= 0.20
    assert clear.any() and (hinges[:, clear] > 0).any(dim=0).all()
    if case.auto_reset:
        first = int(coll[:, 0].float().argmax())
        assert coll[first:, 0].all() and want["terminated"][first:, 0].all() and first < case.K - 1
        assert (want["rows"][first:, 0, 15] < 0).all()                      # the observed clearance is that of the reset pose: inside


def test_without_hit_terminates_the_task_alone_ends_episodes_and_contact_still_fires(gpu_device):
    case, sc, (got, got_state), (want, want_state, _) = flown(IDS[0], 0)
    assert want["collided"].any() and not want["terminated"].any()
    assert all(same(got[k], want[k]) for k in got) and same_state(got_state, want_state)
    ended = flown(IDS[0])[3][0]
    assert ended["terminated"].any() and not same(ended["rows"], want["rows"])


@pytest.mark.parametrize("name", IDS)
def test_with_nothing_near_it_is_gpd_rollout(gpu_device, name):
    """every record 50 m away: the kinematic part of the rows, reward, flags, the final state, counters, last RPMs and controller
    members are `gpd_rollout`'s on the same inputs; nothing collides and every range is max_range"""
    case = next(c for c in yo.CASES if c.name == name)
    sc = yo.scene(case, far=True)
    got, got_state = fused(case, sc, gpu_device)
    core = make_core(case, sc, gpu_device, case.auto_reset)
    obs, rew, term, trunc = core.rollout(torch.as_tensor(sc.actions, device=gpu_device).contiguous())
    torch.cuda.synchronize()
    assert same(got["rows"][..., :12], obs) and same(got["reward"], rew)
    assert same(got["terminated"], term.view(torch.uint8)) and same(got["truncated"], trunc.view(torch.uint8))
    assert same_state(got_state, state_of(core))
    assert not got["collided"].any() and (got["rows"][..., 16:] == yo.MAX_RANGE).all() and (got["rows"][..., 15] > 10.0).all()


# ---- the class ----------------------------------------------------------------------------------------------------------------------------
def course():
    from gym_pybullet_drones_amd import obstacles as ob
    return ob.ObstacleField().sphere((0.0, 0.0, 1.0), 0.15).none().box((0.6, 0.0, 1.0), (0.1, 0.2, 0.3)).cylinder((-0.6, 0.3, 0.5), 0.1, 0.5).floor(0.0)


def make_env(dev, E=70, **kw):
    from gym_pybullet_drones_amd import obstacles as ob
    from gym_pybullet_drones_amd.envs import VectorObstacleAviary
    rng = np.random.default_rng(3)
    start = np.stack([rng.uniform(-1.2, -0.9, E), rng.uniform(-0.4, 0.4, E), rng.uniform(0.8, 1.2, E)], axis=1)
    args = dict(rays=ob.fan(5, 1.5), max_range=2.0, frame="body", hit_reward=-5.0, prox_margin=0.4, prox_weight=1.5, task="none",
                initial_xyzs=start[:, None, :], device=dev)
    args.update(kw)
    return VectorObstacleAviary(E, course(), **args)


def forward(env, speed=1.0):
    a = torch.zeros((env.NUM_ENVS, 1, 4), device=env.device)
    a[..., 0], a[..., 3] = 1.0, speed
    return a


def test_reset_row_is_the_row_of_an_aviary_that_auto_reset_to_that_pose(gpu_device):
    env = make_env(gpu_device)
    assert env.OBS_DIM == 21 and env.ROW_LD == 24
    row0 = env.reset()[0].clone()
    assert row0.shape == (70, 1, 21) and (row0[..., 15] > 0.06).all() and (row0[..., 16:] <= 2.0).all() and (row0[..., 16:] < 2.0).any()
    idx = torch.arange(0, 70, 3, device=gpu_device)
    env.core.positions()[idx] = torch.tensor([0.02, 0.0, 1.0], device=gpu_device)          # inside the sphere: the step ends in contact
    obs, reward, terminated, truncated, info = env.step(forward(env))
    assert info["collided"][idx].all() and terminated[idx].all() and not truncated.any() and int(info["collided"].sum()) == len(idx)
    assert same(obs[idx], row0[idx]) and not same(obs, row0)
    assert (reward[idx] < -5.0).all() and (reward[info["collided"] == 0] > -5.0).all()


def test_rollout_is_k_steps_and_the_outputs_have_the_declared_shapes(gpu_device):
    K = 6
    a, b = make_env(gpu_device), make_env(gpu_device)
    a.reset(), b.reset()
    for env in (a, b):
        env.core.velocities()[:, 0] = 2.0                                                    # towards the course: some arrive within K steps
        env.core.positions()[::4] = torch.tensor([-0.3, 0.0, 1.0], device=gpu_device)
    act = forward(a).unsqueeze(0).repeat(K, 1, 1, 1) + 0.05 * torch.randn((K, 70, 1, 4), generator=torch.Generator().manual_seed(1)).to(gpu_device)
    steps = [[x.clone() if torch.is_tensor(x) else x["collided"].clone() for x in a.step(act[t])] for t in range(K)]
    obs, reward, terminated, truncated, info = b.rollout(act)
    assert obs.shape == (K, 70, 1, 21) and reward.shape == terminated.shape == truncated.shape == info["collided"].shape == (K, 70)
    for t in range(K):
        for got, want in zip((obs[t], reward[t], terminated[t], truncated[t], info["collided"][t]), steps[t]):
            assert same(got.float() if got.dtype == torch.bool else got, want.float() if want.dtype == torch.bool else want), t
    assert info["collided"].any() and not info["collided"].all() and same_state(state_of(a.core), state_of(b.core))
    assert same(a._obs(), b._obs())


def test_adapters_return_the_widths_they_declare(gpu_device):
    from gym_pybullet_drones_amd.envs import GymVectorEnvAdapter, VecEnvAdapter
    env = make_env(gpu_device, E=8, rays=None, task="hover")
    assert env.OBS_DIM == 16
    vec = VecEnvAdapter(env, squeeze=True)
    o = vec.reset()
    assert o.shape == (8,) + vec.observation_space.shape == (8, 16)
    o, r, done, infos = vec.step(np.zeros((8,) + vec.action_space.shape, dtype=np.float32))
    assert o.shape == (8, 16) and r.shape == done.shape == (8,) and len(infos) == 8
    env2 = make_env(gpu_device, E=8)
    gym = GymVectorEnvAdapter(env2)
    o, _ = gym.reset()
    assert o.shape == gym.observation_space.shape == (8, 1, 21) and gym.single_observation_space.shape == (1, 21)
    o, r, term, trunc, infos = gym.step(np.zeros(gym.action_space.shape, dtype=np.float32))
    assert o.shape == (8, 1, 21) and r.shape == term.shape == trunc.shape == (8,)


def test_a_refused_call_leaves_the_state_untouched(gpu_device):
    from gym_pybullet_drones_amd import _native
    env = make_env(gpu_device, E=8)
    env.reset()
    env.step(forward(env))
    before, row = state_of(env.core), env._obs().clone()
    bad = _native.GpdObstTask.from_buffer_copy(env._task)
    bad.n_rays = 65
    q = env._obstacles
    with pytest.raises(_native.GpdError, match="n_rays"):
        env.core.rollout_obst(bad, q.obst, q.n_obst, q.obst_ld, env._rays, forward(env), num_steps=1, last_only=True)
    bad.n_rays, bad.collision_radius = 5, float("nan")
    with pytest.raises(_native.GpdError, match="collision_radius"):
        env.core.rollout_obst(bad, q.obst, q.n_obst, q.obst_ld, env._rays, forward(env), num_steps=1, last_only=True)
    torch.cuda.synchronize()
    assert same_state(before, state_of(env.core)) and same(row, env._obs())
