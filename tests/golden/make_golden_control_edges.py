#!/usr/bin/env python3
"""Generate tests/golden/control_edges_cf2x.npz and control_edges_cf2p.npz: the REFERENCE'S OWN answers on the case tables of
tests/helpers/control_edges.py (the control step at its clips and ties).

Run in the build container only (needs the reference, see make_golden.py):  python tests/golden/make_golden_control_edges.py [out_dir]

The unmodified reference classes run over oracle/pybullet_shim.py, as in make_golden.py; the existing fixtures are not touched.  Inputs
are the tables' float32 values widened to float64; the reference keeps its own float64 coefficients and bounds (0.15, not float32(0.15)),
plus the attribute overrides of control_edges.GAINS on the rows that name them.  Recorded per airframe (inputs and outputs only):
  pid_*     `DSLPIDControl.computeControl` (ctrl_dt = 2^-6) on the DSLPID table: the nine members assigned before the call and read back
            after it, rpm, pos_e, yaw_e
  act_*     `HoverAviary._preprocessAction` (`CtrlAviary`'s for the raw RPMs) on the action-map table, pyb_freq 256 / ctrl_freq 64, the
            cached state assigned the way make_golden.py's force_models does: the RPMs and the controller's members afterwards
  task_*    `_computeReward`, `_computeTerminated`, `_computeTruncated` of `HoverAviary` on the task table's DYADIC rows (x, y, z, the
            counter: there the reference's float64 bound and the device's float32 bound are the same number)
"""
import os
import sys

import numpy as np

from make_golden import HERE, REPO, _silence, load_reference

sys.path.insert(0, os.path.join(REPO, "tests", "helpers"))


def generate(model, ref, ce):
    E = ref["enums"]
    dm = E.DroneModel(model)
    out = {}
    # ---- DSLPIDControl.computeControl
    rows = ce.dslpid_rows(model)
    names = sorted(ce.GAINS)
    rec = {k: [] for k in ("rpm", "pos_e", "yaw_e", "mem_after")}
    for r in rows:
        with _silence():
            c = ref["DSLPIDControl"](drone_model=dm)
        for k, v in ce.GAINS[r.gains].items():
            setattr(c, k, np.array(v) if isinstance(v, tuple) else v)
        m = ce.wide(r.mem)
        c.integral_pos_e, c.last_rpy, c.integral_rpy_e = m[0:3].copy(), m[3:6].copy(), m[6:9].copy()
        rpm, pe, ye = c.computeControl(ce.DT, ce.wide(r.pos), ce.wide(r.quat), ce.wide(r.vel), np.zeros(3), ce.wide(r.tpos), ce.wide(r.trpy),
                                       ce.wide(r.tvel), ce.wide(r.trates))
        rec["rpm"].append(rpm); rec["pos_e"].append(pe); rec["yaw_e"].append(ye)
        rec["mem_after"].append(np.concatenate([c.integral_pos_e, c.last_rpy, c.integral_rpy_e]))
    packed = ce.pack(rows, len(rows))
    out.update({"pid_" + k: v for k, v in packed.items()})
    out["pid_gains"] = np.array([names.index(r.gains) for r in rows], dtype=np.int8)
    out.update({"pid_" + k: np.array(v, dtype=np.float64) for k, v in rec.items()})
    # ---- _preprocessAction
    with _silence():
        probe = ref["CtrlAviary"](drone_model=dm, physics=E.Physics.DYN)
    arows = ce.action_rows(float(np.float32(probe.MAX_RPM)))
    rpm_l, mem_l = [], []
    for r in arows:
        A = ce.ACT_DIM[r.act]
        with _silence():
            if r.act == "raw_rpm":
                env = ref["CtrlAviary"](drone_model=dm, physics=E.Physics.DYN, initial_xyzs=ce.wide(r.pos)[None], pyb_freq=ce.PYB_FREQ,
                                        ctrl_freq=ce.CTRL_FREQ)
            else:
                env = ref["HoverAviary"](drone_model=dm, physics=E.Physics.DYN, act=E.ActionType(r.act), initial_xyzs=ce.wide(r.pos)[None],
                                         pyb_freq=ce.PYB_FREQ, ctrl_freq=ce.CTRL_FREQ)
        env.pos[0], env.quat[0], env.vel[0] = ce.wide(r.pos), ce.wide(r.quat), ce.wide(r.vel)
        env.rpy[0] = ce.bm.euler_from_quaternion(env.quat[0])
        mem = np.zeros(9)
        if r.act in ("pid", "vel", "one_d_pid"):
            c, m = env.ctrl[0], ce.wide(r.mem)
            c.integral_pos_e, c.last_rpy, c.integral_rpy_e = m[0:3].copy(), m[3:6].copy(), m[6:9].copy()
        with np.errstate(all="ignore"):
            rpm_l.append(np.reshape(env._preprocessAction(ce.wide(r.action[:A])[None]), 4))
        if r.act in ("pid", "vel", "one_d_pid"):
            mem = np.concatenate([c.integral_pos_e, c.last_rpy, c.integral_rpy_e])
        mem_l.append(mem)
    out["act_pos"], out["act_quat"], out["act_vel"] = (np.stack([getattr(r, k) for r in arows]) for k in ("pos", "quat", "vel"))
    out["act_action"], out["act_mem"] = np.stack([r.action for r in arows]), np.stack([r.mem for r in arows])
    out["act_type"] = np.array([sorted(ce.ACT_DIM).index(r.act) for r in arows], dtype=np.int8)
    out["act_rpm"], out["act_mem_after"] = np.array(rpm_l, dtype=np.float64), np.array(mem_l, dtype=np.float64)
    # ---- the hover task on the dyadic rows
    trows = [r for r in ce.task_rows() if r.dyadic]
    with _silence():
        env = ref["HoverAviary"](drone_model=dm, physics=E.Physics.DYN, pyb_freq=ce.PYB_FREQ, ctrl_freq=ce.CTRL_FREQ)
    res = []
    for r in trows:
        o = ce.wide(r.obs)
        env.pos[0], env.rpy[0], env.step_counter = o[0:3], o[3:6], r.counter
        res.append((float(env._computeReward()), bool(env._computeTerminated()), bool(env._computeTruncated())))
    out["task_obs"], out["task_counter"] = np.stack([r.obs for r in trows]), np.array([r.counter for r in trows], dtype=np.int32)
    out["task_reward"] = np.array([x[0] for x in res], dtype=np.float64)
    out["task_terminated"], out["task_truncated"] = np.array([x[1] for x in res]), np.array([x[2] for x in res])
    return out


def main(out_dir=HERE):
    _, ref = load_reference()
    import control_edges as ce
    for model in ("cf2x", "cf2p"):
        path = os.path.join(out_dir, f"control_edges_{model}.npz")
        np.savez_compressed(path, **generate(model, ref, ce))
        print(f"wrote {path}  ({os.path.getsize(path) / 1024:.1f} KiB)")


if __name__ == "__main__":
    main(*sys.argv[1:2])
