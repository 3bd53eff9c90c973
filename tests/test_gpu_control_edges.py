"""The control step at its clips and ties on the MI355X: `dslpid`, `map_action` and `task_single` (csrc/gpd_common.inc) through
`gpd_pid` / `gpd_pid_sync`, `gpd_step`, `gpd_rollout` / `gpd_rollout_plant` and `gpd_task_eval`, on the case tables of
tests/helpers/control_edges.py -- every integral landing on, carried past and starting outside its clip, every torque and rotor
saturated and not, the 1 m waypoint step and the zero direction exactly on their compares, the task's bounds on, one float32 step
inside and one beyond -- against the float64 yardstick of that module (oracle/aviary_oracle.py on the float32 inputs, coefficients and
bounds as the device holds them).  NOTHING is masked: every row of every table is in every comparison; flags and classes (which member
sits on which bound, which rotor on which PWM edge) are exact; tests/test_host_control_edges.py holds the conditions that make this
safe (census, margins, `on` rows exact in float64) and pins the yardstick to the reference's own answers.  257 rows per launch.

Errors are in units of the project's CEILING for the quantity -- RPM 0.2; members rtol 1e-5 + atol 2e-6; pos_e rtol 1e-5 + atol 1e-6; yaw_e
rtol 1e-4 + atol 2e-5; kinematics 2e-5 of the row's scale; reward 1e-4 -- and the bounds are 3 x what the MI355X measures (DESIGN.md
section 4), never above 1:
MEASURED (MI355X, the largest over both airframes and every row, as a fraction of the ceiling):
    gpd_pid        rpm 0.300 (0.060 RPM)   members 0.005   pos_e 0 (exact)   yaw_e 0.002
    gpd_pid_sync   rpm 0.007               members 0.005   pos_e 0           yaw_e 0.001
    gpd_step       rpm 0.013               members 0.005   kinematics 0.042  reward 0.002
    gpd_rollout    rpm 0.054               members 0.011   kinematics 0.063            (the third of three steps)
    gpd_task_eval  reward 0.002
BOUND holds 3 x these (3 x the upper end of the last printed digit)."""
import os
import sys

import numpy as np
import pytest
import torch

from conftest import REPO

sys.path.insert(0, os.path.join(REPO, "tests", "helpers"))
import control_edges as ce  # noqa: E402

pytestmark = pytest.mark.gpu

ACT_CODE = {"rpm": 0, "pid": 1, "vel": 2, "one_d_rpm": 3, "one_d_pid": 4, "raw_rpm": 5}
#: rtol, atol of the ceilings
CEIL = {"rpm": (0.0, 0.2), "mem": (1e-5, 2e-6), "pos_e": (1e-5, 1e-6), "yaw_e": (1e-4, 2e-5), "reward": (0.0, 1e-4)}
KIN_CEIL = 2e-5
#: fraction of the ceiling each group may use: 3 x the measured figure in the comment, at most 1
BOUND = {
    # (pos_e: every target_pos - cur_pos of the table is a float32 number, the subtraction is exact: measured 0, bound 0)
    "gpd_pid rpm": 0.91, "gpd_pid mem": 0.017, "gpd_pid pos_e": 0.0, "gpd_pid yaw_e": 0.0075,
    "gpd_pid_sync rpm": 0.023, "gpd_pid_sync mem": 0.017, "gpd_pid_sync pos_e": 0.0, "gpd_pid_sync yaw_e": 0.0045,
    "gpd_step rpm": 0.041, "gpd_step mem": 0.017, "gpd_step kin": 0.13, "gpd_step reward": 0.0075,
    "gpd_rollout rpm": 0.17, "gpd_rollout mem": 0.035, "gpd_rollout kin": 0.19,
    "gpd_task_eval reward": 0.0075,
}
WORST = {}


def record(group, what, got, ref, kind):
    """largest |got - ref| over EVERY element, in units of the ceiling; printed, held to BOUND[group]"""
    got, ref = np.asarray(got, dtype=np.float64), np.asarray(ref, dtype=np.float64)
    assert got.shape == ref.shape and np.isfinite(got).all(), (group, what)
    if kind == "kin":          # [n, 13]: per column, relative to the column's scale (tests/test_gpu_parity.py)
        err = (np.abs(got - ref) / np.maximum(np.abs(ref).max(axis=0, keepdims=True), 1.0)).max() / KIN_CEIL
    else:
        rtol, atol = CEIL[kind]
        err = (np.abs(got - ref) / (atol + rtol * np.abs(ref))).max()
    WORST[group] = max(WORST.get(group, 0.0), float(err))
    print(f"MEASURED {group} [{what}]: {err:.3e} of the ceiling (so far {WORST[group]:.3e}, bound {BOUND[group]})")
    assert err <= BOUND[group], (group, what, err)


def padded(rows, n=ce.PAD):
    return list(rows) + [rows[0]] * (n - len(rows))


def _batch_ctrl(dev, model, gains, n=ce.PAD):
    from gym_pybullet_drones_amd.control import DSLPIDControlBatch
    from gym_pybullet_drones_amd.utils.enums import DroneModel
    ctrl = DSLPIDControlBatch(n, DroneModel(model), device=dev)
    _set_gains(ctrl, gains)
    return ctrl


def _set_gains(ctrl, gains):
    for k, v in ce.GAINS[gains].items():
        setattr(ctrl, k, np.array(v) if isinstance(v, tuple) else v)
    ctrl._coefficients_changed()


def _check_classes(out, ref, c, what):
    """where the yardstick clips a member the device's member IS float32(bound); where it clips a rotor the RPM is within one float32
    step of fma(scale, bound, const)"""
    b = ce.member_bounds(c)
    on = ref["member_clip"] != 0
    want = (ref["member_clip"] * b).astype(np.float32)
    assert np.array_equal(out["mem"][on], want[on]), (what, np.argwhere(out["mem"] != np.where(on, want, out["mem"])))
    for edge, pwm in ((-1, c.MIN_PWM), (1, c.MAX_PWM)):
        at = np.float32(np.float64(np.float32(c.PWM2RPM_SCALE)) * pwm + np.float64(np.float32(c.PWM2RPM_CONST)))
        sel = ref["rotor_clip"] == edge
        assert (np.abs(out["rpm"][sel] - at) <= np.spacing(np.abs(at))).all(), (what, edge)


# ---- gpd_pid ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("model", ["cf2x", "cf2p"])
def test_gpd_pid_on_every_row_of_the_table(gpu_device, model):
    for gains, rs in ce.by_gains(ce.dslpid_rows(model)).items():
        rows = padded(rs)
        a, c = ce.pack(rows), ce.yardstick_ctrl(model, gains)
        ctrl = _batch_ctrl(gpu_device, model, gains)
        ctrl._state[:, :ce.PAD] = torch.as_tensor(a["mem"].T.copy(), device=gpu_device)
        for k, ref in enumerate(ce.run_dslpid(model, gains, rows, calls=2)):      # (the second call: on the members the first one STORED)
            rpm, pe, ye = ctrl.computeControl(ce.DT, a["pos"], a["quat"], a["vel"], None, a["tpos"], a["trpy"], a["tvel"], a["trates"])
            out = dict(rpm=rpm.cpu().numpy(), pos_e=pe.cpu().numpy(), yaw_e=ye.cpu().numpy(), mem=ctrl._state[:, :ce.PAD].t().cpu().numpy())
            what = f"{model} {gains} call {k}"
            for q in ("rpm", "pos_e", "yaw_e", "mem"):
                record("gpd_pid " + q, what, out[q], ref[q], q)
            _check_classes(out, ref, c, what)


@pytest.mark.parametrize("model", ["cf2x", "cf2p"])
def test_gpd_pid_sync_on_a_handful_of_rows(gpu_device, model):
    """the single-drone class (page-locked operands, one library call): the `on`, the carried-past and the outside-start rows, a mixed
    PWM row, a wrap"""
    from gym_pybullet_drones_amd.control import DSLPIDControl
    from gym_pybullet_drones_amd.utils.enums import DroneModel
    rows = ce.dslpid_rows(model)
    want = ("ipx:on+", "ipy:beyond-", "ipz:on-", "ipz2:beyond+", "irx:beyond+", "iry:beyond-", "irz:beyond-", "t1:beyond+", "torques:inside",
            "along:beyond-", "pwm:4max", "pwm:1max", "pwm:3min", "wrap:yaw", "yaw_e:cut")
    for pin in want:
        r = next(r for r in rows if pin in r.pins)
        ctrl = DSLPIDControl(DroneModel(model), device=gpu_device)
        _set_gains(ctrl, r.gains)
        ctrl._state[:, 0] = torch.as_tensor(r.mem)
        ref = ce.run_dslpid(model, r.gains, [r], calls=1)[0]
        rpm, pe, ye = ctrl.computeControl(ce.DT, r.pos, r.quat, r.vel, np.zeros(3), r.tpos, r.trpy, r.tvel, r.trates)
        mem = np.concatenate([ctrl.integral_pos_e, ctrl.last_rpy, ctrl.integral_rpy_e])
        out = dict(rpm=np.float32(rpm)[None], pos_e=pe[None], yaw_e=np.array([ye]), mem=np.float32(mem)[None])
        for q in ("rpm", "pos_e", "yaw_e", "mem"):
            record("gpd_pid_sync " + q, f"{model} {r.name}", out[q], ref[q], q)
        _check_classes(out, ref, ce.yardstick_ctrl(model, r.gains), r.name)


@pytest.mark.parametrize("model", ["cf2x", "cf2p"])
def test_singular_inputs_stay_finite_inside_the_clips(gpu_device, model):
    """desired force zero / parallel to the heading: the reference answers NaN.  include/gpd.h (gpd_pid) promises finite RPMs inside
    [rpm(MIN_PWM), rpm(MAX_PWM)] and finite members inside their clips -- a clip of a NaN is one of its bounds --, pos_e as ever, and
    nothing about yaw_e; a second call on ordinary inputs is ordinary again"""
    rows = padded(ce.singular_rows(model), 64 + 3)
    a, c = ce.pack(rows, len(rows)), ce.yardstick_ctrl(model)
    ctrl = _batch_ctrl(gpu_device, model, "default", len(rows))
    rpm, pe, _ = ctrl.computeControl(ce.DT, a["pos"], a["quat"], a["vel"], None, a["tpos"], a["trpy"], a["tvel"], a["trates"])
    rpm, mem = rpm.cpu().numpy().astype(np.float64), ctrl._state[:, :len(rows)].t().cpu().numpy().astype(np.float64)
    lo, hi = (c.PWM2RPM_SCALE * p + c.PWM2RPM_CONST for p in (c.MIN_PWM, c.MAX_PWM))
    assert np.isfinite(rpm).all() and (rpm >= lo - 0.01).all() and (rpm <= hi + 0.01).all()
    b = ce.member_bounds(c)
    b[3:6] = np.pi
    assert np.isfinite(mem).all() and (np.abs(mem) <= b * (1 + 1e-6)).all()
    np.testing.assert_array_equal(pe.cpu().numpy(), a["tpos"] - a["pos"])
    hover = padded([ce.dslpid_rows(model)[0]], len(rows))
    h = ce.pack(hover, len(rows))
    ctrl._state[3:6] = 0.0
    ctrl._state[6:9] = 0.0          # (the attitude integrals came back as bounds: start the ordinary call from zero)
    ctrl._state[0:3] = 0.0
    rpm2, _, _ = ctrl.computeControl(ce.DT, h["pos"], h["quat"], h["vel"], None, h["tpos"], h["trpy"], h["tvel"], h["trates"])
    ref = ce.run_dslpid(model, "default", hover[:1], calls=1)[0]
    assert np.abs(rpm2.cpu().numpy() - ref["rpm"][0]).max() <= 0.2


# ---- gpd_step / gpd_rollout on the action map ---------------------------------------------------------------------------------------------
def _core(dev, act, rows, D=1, task=1, model="cf2x", keep_term=False, **kw):
    from gym_pybullet_drones_amd import engine
    from gym_pybullet_drones_amd.utils.enums import DroneModel
    n = len(rows)
    kin, pid, actions = ce.pack_actions(rows)
    core = engine.SimCore(drone_model=DroneModel(model), num_envs=n // D, drones_per_env=D, physics=0, pyb_freq=ce.PYB_FREQ,
                          ctrl_freq=ce.CTRL_FREQ, act_code=ACT_CODE[act], task=task, initial_xyzs=kin[0:3].T.reshape(n // D, D, 3),
                          target_pos=np.broadcast_to(np.array(ce.TARGET), (D, 3)), xy_bound=ce.XY_BOUND, z_bound=ce.Z_BOUND, tilt_bound=0.4,
                          term_dist=ce.TERM_DIST, episode_len_sec=ce.EPISODE_LEN_SEC, track_rpm=True, keep_terminal_obs=keep_term,
                          device=dev, **kw)
    assert core._cfg.tilt_bound == ce.TILT_BOUND and core._cfg.trunc_counter == ce.TRUNC_COUNTER
    _load(core, kin, pid)
    return core, torch.as_tensor(actions, device=dev)


def _load(core, kin, pid, counter=None):
    core.set_state(kin=kin, step_counter=np.zeros(core.E, dtype=np.int32) if counter is None else counter)
    if core.pid is not None:
        core.set_state(pid=pid)


def _state_of(core):
    n = core.N
    out = dict(kin=core.kin[:, :n].t().cpu().numpy(), rpm=core.last_rpm[:, :n].t().cpu().numpy())
    if core.pid is not None:
        out["mem"] = core.pid[:, :n].t().cpu().numpy()
    return out


def _rows_for(act):
    from oracle.aviary_oracle import UrdfConstants
    rows = [r for r in ce.action_rows(float(np.float32(UrdfConstants(ce.urdf("cf2x"), "cf2x").MAX_RPM))) if r.act == act]
    if act == "pid":
        rows += list(ce.dslpid_as_waypoints(ce.dslpid_rows("cf2x")))
    return rows


def _compare_step(group, what, got, ref, pid):
    record(group + " kin", what, got["kin"], ref["kin"], "kin")
    record(group + " rpm", what, got["rpm"], ref["rpm"], "rpm")
    if pid:
        record(group + " mem", what, got["mem"], ref["mem"], "mem")


@pytest.mark.parametrize("act", ["pid", "vel", "one_d_pid", "raw_rpm", "rpm", "one_d_rpm"])
def test_gpd_step_on_the_action_map(gpu_device, act):
    """one env step from the table's state: last_rpm, the members and the kinematics, every row"""
    rows = padded(_rows_for(act))
    core, actions = _core(gpu_device, act, rows)
    core.step(actions)
    got, ref = _state_of(core), ce.run_steps("cf2x", act, rows)[0]
    pid = act in ("pid", "vel", "one_d_pid")
    _compare_step("gpd_step", act, got, ref, pid)
    record("gpd_step reward", act, core.reward.cpu().numpy(), ref["reward"], "reward")
    assert np.isfinite(got["kin"]).all() and np.isfinite(got["rpm"]).all()
    if act == "pid":
        # exactly on the 1 m compare the drone is sent to the waypoint ITSELF: e = fl(act - pos), e * 2^-6 exact, the member is the
        # yardstick's bit for bit.  On the tie row float64 sees 1 + 2^-24 and steps; the unit step lands on the same member
        for i, r in enumerate(rows):
            if r.pins[0] in ("wp:on", "wp:tie"):
                assert np.array_equal(got["mem"][i, 0:3], ref["mem"][i, 0:3].astype(np.float32)), r.name
        b = ce.member_bounds(ce.yardstick_ctrl("cf2x"))
        for i, (r, cl) in enumerate(zip(rows, ref["classes"])):
            for j, n in ((0, "ipx"), (1, "ipy"), (2, "ipz")):
                if cl[n] != "inside":
                    assert got["mem"][i, j] == np.float32(b[j]) * (1 if cl[n].endswith("+") else -1), (r.name, n)
    if act == "vel":
        # the contract of include/gpd.h (GPD_ACT_VEL): all three components +-0 is the only zero direction
        still = ce.run_steps("cf2x", act, [r for r in rows if r.pins[0] == "vel:zero"][:1])[0]["rpm"][0]
        for i, r in enumerate(rows):
            if r.pins[0] == "vel:zero":
                assert np.abs(got["rpm"][i] - still).max() <= 0.2
            if r.pins[0] == "vel:tiny":
                assert np.abs(got["rpm"][i] - still).max() > 100.0, r.name       # it flies: 0.25 m/s asked of a drone at rest


def test_gpd_step_multihover_three_drones(gpu_device):
    """the PID rows as aviaries of three drones (the MULTI kernels; no force couples the drones at physics 0)"""
    rows = padded(_rows_for("pid"), 258)
    core, actions = _core(gpu_device, "pid", rows, D=3, task=2)
    core.step(actions)
    _compare_step("gpd_step", "pid D=3", _state_of(core), ce.run_steps("cf2x", "pid", rows)[0], True)


@pytest.mark.parametrize("keep_term", [False, True], ids=["rollout1", "rollout-with-terminal-obs"])
@pytest.mark.parametrize("act", ["pid", "vel", "one_d_pid", "raw_rpm"])
def test_gpd_rollout_three_steps(gpu_device, act, keep_term):
    """K = 3 with the action held: bit for bit three single steps, within the bounds of the yardstick's three steps, and the same bits
    from gpd_rollout_plant with an all-ones table"""
    rows, K = padded(_rows_for(act)), 3
    pid = act in ("pid", "vel", "one_d_pid")
    a, actions = _core(gpu_device, act, rows, keep_term=keep_term)
    b, _ = _core(gpu_device, act, rows, keep_term=keep_term)
    p, _ = _core(gpu_device, act, rows, keep_term=keep_term)
    p.set_plant(torch.ones((9, p.E), device=gpu_device))
    ref = ce.run_steps("cf2x", act, rows, K=K)
    singles = []
    for k in range(K):
        o, rw, te, tr = a.step(actions)
        singles.append((o.clone(), rw.clone(), te.clone(), tr.clone()))
        if k == K - 1:
            _compare_step("gpd_rollout", f"{act} step {k}", _state_of(a), ref[k], pid)
    acts = actions.unsqueeze(0).repeat(K, 1, 1).contiguous()
    for other in (b, p):
        ob, rb, teb, trb = other.rollout(acts)
        for k in range(K):
            for x, y in zip(singles[k], (ob[k], rb[k], teb[k], trb[k])):
                assert torch.equal(x.reshape(-1), y.reshape(-1)), (act, k)
        assert torch.equal(a.kin, other.kin) and torch.equal(a.last_rpm, other.last_rpm) and torch.equal(a.step_counter, other.step_counter)
        assert not pid or torch.equal(a.pid, other.pid)


# ---- the task ---------------------------------------------------------------------------------------------------------------------------------
def _exact_rewards(rows, rew):
    for i, r in enumerate(rows):
        for pin, v in (("reward:2", 2.0), ("reward:1", 1.0), ("reward:0", 0.0)):
            if pin in r.pins:
                assert rew[i] == v, (r.name, rew[i])


def test_gpd_task_eval_on_every_row_flags_exact(gpu_device):
    rows = padded(ce.task_rows())
    obs, cnt = np.stack([r.obs for r in rows]), np.array([r.counter for r in rows], dtype=np.int32)
    core, _ = _core(gpu_device, "rpm", padded(ce.tilt_step_rows()))
    rew, term, trunc = core.task_eval(torch.as_tensor(obs, device=gpu_device), torch.as_tensor(cnt, device=gpu_device))
    r64, t64, tr64, _ = ce.task_f64(obs, cnt)
    record("gpd_task_eval reward", "rows", rew.cpu().numpy(), r64, "reward")
    _exact_rewards(rows, rew.cpu().numpy())
    bad = np.flatnonzero((term.cpu().numpy() != t64) | (trunc.cpu().numpy() != tr64))
    assert bad.size == 0, [rows[i].name for i in bad]


def test_gpd_step_decides_the_task_rows_as_gpd_task_eval_does(gpu_device):
    """the rows a hover step leaves exactly in place (x, y, z, the distance to the target, the counter), as the state a level drone at
    hover RPMs starts from; the tilt bound 2e-3 to either side (the angle comes out of the quaternion here)"""
    trows = [r for r in ce.task_rows() if r.via_step]
    arows = [ce._arow(r.name, r.pins, "rpm", (0, 0, 0, 0), r.obs[0:3]) for r in trows] + list(ce.tilt_step_rows())
    cnt = np.array([r.counter for r in trows] + [0] * (ce.PAD - len(trows)), dtype=np.int32)
    rows = padded(arows)
    core, actions = _core(gpu_device, "rpm", rows)
    kin, pid, _ = ce.pack_actions(rows)
    _load(core, kin, pid, cnt)
    _, rew, term, trunc = core.step(actions)
    got = _state_of(core)
    level = np.array([i < len(trows) or i >= len(arows) for i in range(ce.PAD)])
    assert np.array_equal(got["kin"][level, 0:3], kin[0:3].T[level]), "a hover step moved a level drone at rest"
    obs = np.zeros((ce.PAD, 12), dtype=np.float32)
    obs[:, 0:3] = got["kin"][:, 0:3]         # (the tilted drones drift: the task sees where they are now)
    for i, r in enumerate(rows):
        obs[i, 3:6] = ce._quat_rpy((0, 0, 0))[1] if i < len(trows) else ce.bm.euler_from_quaternion(r.quat.astype(np.float64))
    r64, t64, tr64, _ = ce.task_f64(obs, cnt)
    record("gpd_step reward", "task rows", rew.cpu().numpy(), r64, "reward")
    bad = np.flatnonzero((term.cpu().numpy() != t64) | (trunc.cpu().numpy() != tr64))
    assert bad.size == 0, [rows[i].name for i in bad]
    assert tr64.any() and t64.any() and not tr64.all()
    np.testing.assert_array_equal(core.step_counter.cpu().numpy(), cnt + ce.PYB_FREQ // ce.CTRL_FREQ)
