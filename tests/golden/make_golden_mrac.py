#!/usr/bin/env python3
"""Generate the MRAC fixtures in tests/golden/ by running the REFERENCE'S OWN `control/MRAC.py` and `CtrlAviary`.

Run in the build container only (needs the reference, see make_golden.py):  python tests/golden/make_golden_mrac.py

The reference's `MRAC` imports python-control for one call, `ct.place(A, B, poles)`; python-control implements it as
`scipy.signal.place_poles(A, B, poles, method="YT").gain_matrix`, so a stand-in module `control` with exactly that function is
installed before the UNMODIFIED reference classes are imported.  Written, for cf2x and cf2p:

  mrac_design_<m>.npz   A, B, K, Am, Bm, P, Kr_ref_gain, Kx0 of the reference's `_compute_K` (A, B and K are rebuilt here with the
                        reference's own statements, `:69-92`: the class does not keep them)
  mrac_hover_<m>.npz    the closed loop of the reference's example (`examples/mrac.py:80-90`) on `CtrlAviary(physics=DYN,
                        pyb_freq=240, ctrl_freq=120)`, start (0, 0, 0.5), target (0.3, -0.2, 1.0), 720 control steps: the state vector,
                        the RPMs and Kx, Kr, Xm after every step
  mrac_calls_<m>.npz    complete operands and results of every 10th call of that run (adapted gains included) plus 64 calls on
                        random states with |rpy| < 0.5 rad, random gains around the design's and random model states
  mrac_calls_wide_<m>.npz   64 more single calls at attitudes in every quadrant of roll and yaw, |pitch| up to 1.5 rad
  mrac_hover_cf2x_mass120.npz   the same loop with the instance's M and GRAVITY x 1.2 (the controller stays nominal)

The scenario is the one the reference's controller flies: it converges from (0, 0, 0.5); a start on z = 0 under Physics.DYN, or a 2 m
step, saturates its PWM clip for hundreds of steps and diverges -- no fixture there.
"""
import os
import sys
import types

import numpy as np

from make_golden import HERE, _silence, load_reference

STEPS, EVERY, RANDOM_CALLS, SEED = 720, 10, 64, 11
START, TARGET = np.array([[0.0, 0.0, 0.5]]), np.array([0.3, -0.2, 1.0])


def install_control_stand_in():
    from scipy.signal import place_poles
    ct = types.ModuleType("control")
    ct.place = lambda A, B, p: place_poles(A, B, p, method="YT").gain_matrix
    sys.modules["control"] = ct


def members(c):
    return np.array(c.Kx, dtype=np.float64).copy(), np.array(c.Kr, dtype=np.float64).copy(), np.array(c.Xm, dtype=np.float64).reshape(12).copy()


def call(c, dt, op):
    """one `computeControl` with everything it reads and leaves behind"""
    kx, kr, xm = members(c)
    rec = dict(op, dt=dt, Kx_in=kx, Kr_in=kr, Xm_in=xm, counter_in=np.int64(c.control_counter))
    rpm, pos_e, rpy_e = c.computeControl(control_timestep=dt, cur_pos=op["cur_pos"], cur_quat=op["cur_quat"], cur_vel=op["cur_vel"],
                                         cur_ang_vel=op["cur_ang_vel"], target_pos=op["target_pos"], target_rpy=op["target_rpy"],
                                         target_vel=op["target_vel"], target_rpy_rates=op["target_rpy_rates"])
    kx, kr, xm = members(c)
    rec.update(rpm=np.array(rpm, dtype=np.float64), pos_e=np.array(pos_e, dtype=np.float64), rpy_e=np.array(rpy_e, dtype=np.float64),
               Kx_out=kx, Kr_out=kr, Xm_out=xm)
    return rec


def hover(ref, MRAC, model, mass_scale=1.0, keep_calls=False):
    E = ref["enums"]
    with _silence():
        env = ref["CtrlAviary"](drone_model=model, num_drones=1, initial_xyzs=START, initial_rpys=np.zeros((1, 3)),
                                physics=E.Physics.DYN, pyb_freq=240, ctrl_freq=120)
        env.reset(seed=0)
        ctrl = MRAC(drone_model=model)
    env.M *= mass_scale
    env.GRAVITY *= mass_scale
    dt = env.CTRL_TIMESTEP
    action = np.zeros((1, 4))
    state, rpm, Kx, Kr, Xm, calls = [], [], [], [], [], []
    zero = np.zeros(3)
    for i in range(STEPS):
        obs, _, _, _, _ = env.step(action)
        s = np.array(obs[0], dtype=np.float64)
        op = dict(cur_pos=s[0:3], cur_quat=s[3:7], cur_vel=s[10:13], cur_ang_vel=s[13:16], target_pos=TARGET, target_rpy=zero,
                  target_vel=zero, target_rpy_rates=zero)
        rec = call(ctrl, dt, op)          # (= computeControlFromState(state=obs[0], ...), `control/BaseControl.py:62-101`)
        action[0, :] = rec["rpm"]
        state.append(s), rpm.append(rec["rpm"]), Kx.append(rec["Kx_out"]), Kr.append(rec["Kr_out"]), Xm.append(rec["Xm_out"])
        if keep_calls and i % EVERY == 0:
            calls.append(rec)
    out = dict(state20=np.array(state), rpm=np.array(rpm), Kx=np.array(Kx), Kr=np.array(Kr), Xm=np.array(Xm), start=START[0], target=TARGET,
               mass_scale=np.float64(mass_scale), pyb_freq=np.int64(240), ctrl_freq=np.int64(120))
    return out, calls, ctrl


def wide_angles(rng, i):
    """attitudes in every quadrant of roll and yaw (the body-rate rotation's sines and cosines change roles and signs there): the
    first calls sit 0.01 .. 0.05 rad beside +-pi/4, +-pi/2, +-3pi/4 and +-pi, the rest are uniform; pitch stays inside +-1.5 (its
    range is +-pi/2) and nothing comes closer than 0.01 rad to the +-pi seam of the Euler extraction"""
    marks = np.array([-np.pi, -0.75 * np.pi, -0.5 * np.pi, -0.25 * np.pi, 0.25 * np.pi, 0.5 * np.pi, 0.75 * np.pi, np.pi])
    if i < 32:
        roll = marks[i % 8] + (0.01 + 0.04 * rng.uniform()) * (1 if marks[i % 8] < 0 else -1) * (1 if abs(marks[i % 8]) > 3 or i < 16 else -1)
        yaw = marks[(i * 3 + 1) % 8] + (0.01 + 0.04 * rng.uniform()) * (1 if marks[(i * 3 + 1) % 8] < 0 else -1)
    else:
        roll, yaw = rng.uniform(-np.pi + 0.01, np.pi - 0.01, 2)
    return np.array([roll, rng.uniform(-1.5, 1.5), yaw])


def random_calls(MRAC, model, rng, wide=False):
    with _silence():
        ctrl = MRAC(drone_model=model)
    kx0, kr0 = np.array(ctrl.Kx).copy(), np.array(ctrl.Kr).copy()
    recs = []
    for i in range(RANDOM_CALLS):
        rpy = wide_angles(rng, i) if wide else rng.uniform(-0.5, 0.5, 3)
        h = rpy / 2
        cr, sr, cp, sp, cy, sy = np.cos(h[0]), np.sin(h[0]), np.cos(h[1]), np.sin(h[1]), np.cos(h[2]), np.sin(h[2])
        quat = np.array([sr * cp * cy - cr * sp * sy, cr * sp * cy + sr * cp * sy, cr * cp * sy - sr * sp * cy, cr * cp * cy + sr * sp * sy])
        pos = rng.uniform(-1, 1, 3) + np.array([0, 0, 1.0])
        op = dict(cur_pos=pos, cur_quat=quat, cur_vel=rng.uniform(-1, 1, 3), cur_ang_vel=rng.uniform(-2, 2, 3),
                  target_pos=pos + rng.uniform(-0.5, 0.5, 3), target_rpy=rng.uniform(-0.2, 0.2, 3), target_vel=rng.uniform(-0.3, 0.3, 3),
                  target_rpy_rates=rng.uniform(-0.3, 0.3, 3))
        ctrl.Kx = kx0 * (1 + 0.05 * rng.uniform(-1, 1, kx0.shape))
        ctrl.Kr = kr0 + 0.05 * rng.uniform(-1, 1, kr0.shape)
        ctrl.control_counter = 0 if i % 8 == 0 else int(rng.integers(1, 1000))     # (counter 0: this call re-seeds Xm)
        ctrl.Xm = (np.hstack([pos, rpy, op["cur_vel"], op["cur_ang_vel"]]) + 0.05 * rng.uniform(-1, 1, 12)).reshape(12, 1)
        recs.append(call(ctrl, 1.0 / 120.0, op))
    return recs


def stack(recs):
    return {k: np.array([r[k] for r in recs]) for k in recs[0]}


def main():
    install_control_stand_in()
    _, ref = load_reference()
    from gym_pybullet_drones.control.MRAC import MRAC
    E = ref["enums"]
    rng = np.random.default_rng(SEED)
    for name, model in (("cf2x", E.DroneModel.CF2X), ("cf2p", E.DroneModel.CF2P)):
        run, calls, ctrl = hover(ref, MRAC, model, keep_calls=True)
        with _silence():
            fresh = MRAC(drone_model=model)
            again = MRAC(drone_model=model)
        assert np.array_equal(fresh.Kx, again.Kx) and np.array_equal(fresh.P, again.P), "the design is not deterministic here"
        # A, B, K with the reference's own statements (`:69-92`, psi = 0)
        g = fresh.g
        a_sub = np.vstack((np.array([[0, 0, 0, g * np.sin(0), g * np.cos(0), 0], [0, 0, 0, -g * np.cos(0), g * np.sin(0), 0]]), np.zeros((4, 6))))
        A = np.block([[np.zeros((6, 6)), np.eye(6)], [a_sub, np.zeros((6, 6))]])
        B = np.vstack((np.zeros((8, 4)), np.diag([1 / fresh.mass, 1 / fresh.Ixx, 1 / fresh.Iyy, 1 / fresh.Izz])))
        K = -np.array(fresh.Kx).T
        assert np.array_equal(fresh.Am, A - B @ K) and np.array_equal(fresh.Bm, B)
        out = os.path.join(HERE, f"mrac_design_{name}.npz")
        np.savez_compressed(out, A=A, B=B, K=K, Am=fresh.Am, Bm=fresh.Bm, P=fresh.P, Kr_ref_gain=fresh.Kr_ref_gain, Kx0=np.array(fresh.Kx),
                            Kr0=np.array(fresh.Kr), gamma=np.float64(fresh.Gamma_x[0, 0]), mixer=np.array(fresh.MIXER_MATRIX, dtype=np.float64),
                            KF=np.float64(fresh.KF))
        err = np.linalg.norm(run["state20"][-1, 0:3] - TARGET)
        print(f"wrote {out} ({os.path.getsize(out)} B)")
        out = os.path.join(HERE, f"mrac_hover_{name}.npz")
        np.savez_compressed(out, **run)
        print(f"wrote {out} ({os.path.getsize(out)} B): position error after {STEPS} steps {err:.4f} m")
        out = os.path.join(HERE, f"mrac_calls_{name}.npz")
        recs = calls + random_calls(MRAC, model, rng)
        np.savez_compressed(out, n_hover=np.int64(len(calls)), **stack(recs))
        print(f"wrote {out} ({os.path.getsize(out)} B): {len(calls)} calls of the run + {RANDOM_CALLS} random")
    # single calls at attitudes far from level (no closed-loop claim there: the reference's design does not fly them)
    wide_rng = np.random.default_rng(SEED + 1)
    for name, model in (("cf2x", E.DroneModel.CF2X), ("cf2p", E.DroneModel.CF2P)):
        recs = stack(random_calls(MRAC, model, wide_rng, wide=True))
        out = os.path.join(HERE, f"mrac_calls_wide_{name}.npz")
        np.savez_compressed(out, n_hover=np.int64(0), **recs)
        print(f"wrote {out} ({os.path.getsize(out)} B): {RANDOM_CALLS} calls, |roll|, |yaw| up to pi - 0.01, |pitch| up to 1.5")
    run, _, _ = hover(ref, MRAC, E.DroneModel.CF2X, mass_scale=1.2)
    out = os.path.join(HERE, "mrac_hover_cf2x_mass120.npz")
    np.savez_compressed(out, **run)
    print(f"wrote {out} ({os.path.getsize(out)} B): position error after {STEPS} steps "
          f"{np.linalg.norm(run['state20'][-1, 0:3] - TARGET):.4f} m")


if __name__ == "__main__":
    main()
