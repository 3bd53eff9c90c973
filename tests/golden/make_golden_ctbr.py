#!/usr/bin/env python3
"""Generate tests/golden/ctbr_calls.npz by running the REFERENCE'S OWN `control/CTBRControl.py`.

Run in the build container only (needs the reference, see make_golden.py):  python tests/golden/make_golden_ctbr.py

The reference's class imports five functions of `transforms3d`, which is not installed here.  A stand-in module with exactly those five,
written from that library's documented behaviour, is installed before the UNMODIFIED reference class is imported:
  quaternions.qmult(q1, q2)        Hamilton product of (w, x, y, z) quaternions
  quaternions.qconjugate(q)        (w, -x, -y, -z)
  quaternions.rotate_vector(v, q)  the vector part of q (0, v) q*  -- no normalisation of q
  quaternions.mat2quat(M)          Bar-Itzhack's method: the eigenvector of the symmetric 4 x 4 matrix K(M) / 3 with the largest
                                   eigenvalue, as (w, x, y, z) with w >= 0
  utils.normalized_vector(v)       v / sqrt(sum(v^2))

Written: ctbr_calls.npz -- operands and results of 256 calls (seeded) on CF2X:
  calls 0..127     attitude within 0.5 rad of level (a random axis, angle U(0, 0.5))
  calls 128..255   attitude anywhere up to 3.1 rad
  even calls go through `computeControl` (cur_quat as (w, x, y, z), the method's own convention), odd ones through
  `computeControlFromState` (a 20-float state vector, quaternion x, y, z, w at 3:7).  The file holds the quaternion in the STATE's order.
  target_rpy / target_rpy_rates are random too: the reference ignores them.
A call with |q_err.w| < 1e-3 (the sign of the rates flips there) or |y^ x z_b| < 1e-2 (the target frame degenerates) is redrawn.
"""
import os
import sys
import types

import numpy as np

from make_golden import HERE, _silence, load_reference

CALLS, SEED = 256, 23


def install_transforms3d_stand_in():
    def qmult(q1, q2):
        w1, x1, y1, z1 = q1
        w2, x2, y2, z2 = q2
        return np.array([w1 * w2 - x1 * x2 - y1 * y2 - z1 * z2, w1 * x2 + x1 * w2 + y1 * z2 - z1 * y2,
                         w1 * y2 - x1 * z2 + y1 * w2 + z1 * x2, w1 * z2 + x1 * y2 - y1 * x2 + z1 * w2])

    def qconjugate(q):
        return np.array(q, dtype=np.float64) * np.array([1.0, -1.0, -1.0, -1.0])

    def rotate_vector(v, q):
        return qmult(q, qmult(np.concatenate([[0.0], v]), qconjugate(q)))[1:]

    def mat2quat(M):
        (xx, xy, xz), (yx, yy, yz), (zx, zy, zz) = np.asarray(M, dtype=np.float64)
        K = np.array([[xx - yy - zz, 0, 0, 0], [yx + xy, yy - xx - zz, 0, 0], [zx + xz, zy + yz, zz - xx - yy, 0],
                      [zy - yz, xz - zx, yx - xy, xx + yy + zz]]) / 3.0      # (names are row, column: zy = M[2][1])
        vals, vecs = np.linalg.eigh(K)               # (reads the lower triangle)
        q = vecs[[3, 0, 1, 2], np.argmax(vals)]
        return -q if q[0] < 0 else q

    def normalized_vector(v):
        v = np.asarray(v, dtype=np.float64)
        return v / np.sqrt(np.sum(v ** 2))

    t3, t3q, t3u = types.ModuleType("transforms3d"), types.ModuleType("transforms3d.quaternions"), types.ModuleType("transforms3d.utils")
    t3q.qmult, t3q.qconjugate, t3q.rotate_vector, t3q.mat2quat = qmult, qconjugate, rotate_vector, mat2quat
    t3u.normalized_vector = normalized_vector
    t3.quaternions, t3.utils = t3q, t3u
    sys.modules.update({"transforms3d": t3, "transforms3d.quaternions": t3q, "transforms3d.utils": t3u})
    return t3q


def main():
    _, ref = load_reference()
    t3q = install_transforms3d_stand_in()
    from gym_pybullet_drones.control.CTBRControl import CTBRControl
    with _silence():
        ctrl = CTBRControl(drone_model=ref["enums"].DroneModel.CF2X)
    rng = np.random.default_rng(SEED)
    recs, redrawn = [], 0
    while len(recs) < CALLS:
        i = len(recs)
        axis = rng.normal(size=3)
        axis /= np.linalg.norm(axis)
        angle = rng.uniform(0.0, 0.5 if i < CALLS // 2 else 3.1)
        xyzw = np.concatenate([np.sin(angle / 2) * axis, [np.cos(angle / 2)]])
        pos = rng.uniform(-1.0, 1.0, 3) + np.array([0.0, 0.0, 1.0])
        op = dict(cur_pos=pos, cur_quat=xyzw, cur_vel=rng.normal(0.0, 0.5, 3), cur_ang_vel=rng.normal(0.0, 1.0, 3),
                  target_pos=pos + rng.uniform(-0.5, 0.5, 3), target_rpy=rng.uniform(-0.3, 0.3, 3),
                  target_vel=rng.normal(0.0, 0.3, 3) * (i % 4 < 2), target_rpy_rates=rng.normal(0.0, 0.3, 3))
        # the two quantities whose smallness makes a call ill-conditioned, from the reference's own statements
        wxyz = np.array([xyzw[3], xyzw[0], xyzw[1], xyzw[2]])
        tar_acc = np.array([3.0, 3.0, 8.0]) * (op["target_pos"] - pos) + np.array([2.5, 2.5, 5.0]) * (op["target_vel"] - op["cur_vel"]) + np.array([0, 0, 9.8])
        zb = tar_acc / np.linalg.norm(tar_acc)
        cross = np.cross([0.0, 1.0, 0.0], zb)
        xb = cross / np.linalg.norm(cross)
        yb = np.cross(zb, xb)
        q_err = t3q.qmult(t3q.qconjugate(wxyz), t3q.mat2quat(np.vstack([xb, yb / np.linalg.norm(yb), zb]).T))
        if abs(q_err[0]) < 1e-3 or np.linalg.norm(cross) < 1e-2:
            redrawn += 1
            continue
        via_state = i % 2 == 1
        if via_state:
            state = np.concatenate([pos, xyzw, np.zeros(3), op["cur_vel"], op["cur_ang_vel"], np.zeros(4)])
            out = ctrl.computeControlFromState(control_timestep=1 / 48, state=state, target_pos=op["target_pos"], target_rpy=op["target_rpy"],
                                               target_vel=op["target_vel"], target_rpy_rates=op["target_rpy_rates"])
        else:
            out = ctrl.computeControl(control_timestep=1 / 48, cur_pos=pos, cur_quat=wxyz, cur_vel=op["cur_vel"], cur_ang_vel=op["cur_ang_vel"],
                                      target_pos=op["target_pos"], target_rpy=op["target_rpy"], target_vel=op["target_vel"],
                                      target_rpy_rates=op["target_rpy_rates"])
        recs.append(dict(op, cmd=np.array(out, dtype=np.float64), via_state=np.bool_(via_state), angle=angle, q_err_w=q_err[0]))
    out = {k: np.array([r[k] for r in recs]) for k in recs[0]}
    np.savez_compressed(os.path.join(HERE, "ctbr_calls.npz"), **out)
    print(f"ctbr_calls.npz: {CALLS} calls, {redrawn} redrawn; min |q_err.w| {np.abs(out['q_err_w']).min():.3g}; |cmd| max {np.abs(out['cmd']).max(axis=0)}")


if __name__ == "__main__":
    main()
