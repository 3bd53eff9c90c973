"""The yardstick of the thrust-and-body-rate controller (include/gpd.h gpd_ctbr / gpd_rollout_ctbr): a float64 numpy restatement of
(a) the outer loop -- the reference's `CTBRControl.computeControl` --, (b) the rate loop of csrc/ctbr_math.inc, written from its
definition in DESIGN.md section 3.17, and the closed loop of both over the oracle's explicit integrator (oracle/batched_oracle.py,
imported, not modified).  Batched over drones: arrays are [n, k].  (a) is checked against the recorded calls of the reference
(tests/test_host_ctbr.py)."""
import os
import sys

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
if REPO not in sys.path:
    sys.path.insert(0, REPO)
from oracle import bullet_math as bm  # noqa: E402
from oracle.aviary_oracle import UrdfConstants  # noqa: E402
from oracle.batched_oracle import BatchedAviary  # noqa: E402

G_Z, K_P, K_D, K_RATES = 9.8, np.array([3.0, 3.0, 8.0]), np.array([2.5, 2.5, 5.0]), np.array([5.0, 5.0, 1.0])
K_RATE, THRUST_MAX, RATE_MAX = np.array([40.0, 40.0, 20.0]), 40.9, 2.0 * np.pi
URDF = {m: os.path.join(REPO, "gym_pybullet_drones_amd", "assets", f"{m}.urdf") for m in ("cf2x", "cf2p", "racer")}


def rel_err(x, ref):
    """the project's metric: max|x - ref| / max(max|ref|, 1)"""
    x, ref = np.asarray(x, dtype=np.float64), np.asarray(ref, dtype=np.float64)
    return float(np.max(np.abs(x - ref)) / max(float(np.max(np.abs(ref))), 1.0))


def _unit(v):
    return v / np.linalg.norm(v, axis=-1, keepdims=True)


def _rot(q):
    """[n, 3, 3] of quaternions x, y, z, w WITHOUT normalisation: v -> q v q*"""
    x, y, z, w = (q[..., i] for i in range(4))
    return np.stack([np.stack([w * w + x * x - y * y - z * z, 2 * (x * y - w * z), 2 * (x * z + w * y)], -1),
                     np.stack([2 * (x * y + w * z), w * w - x * x + y * y - z * z, 2 * (y * z - w * x)], -1),
                     np.stack([2 * (x * z - w * y), 2 * (y * z + w * x), w * w - x * x - y * y + z * z], -1)], -2)


def outer(pos, quat, vel, target_pos, target_vel=None):
    """(a): -> cmd [n, 4] = thrust [m/s^2] | body rates [rad/s]; quat x, y, z, w.  The attitude error is taken on rotation MATRICES
    (R_e = R^T R_t; for its quaternion (w, v): vee(R_e - R_e^T) = 4 w v, trace = 4 w^2 - 1), so no matrix-to-quaternion case analysis:
    2 K w v / |w| ... computed as K vee / (2 |w|) -- the reference's  2 K q_e.xyz sign(q_e.w)."""
    pos, quat, vel, target_pos = (np.asarray(a, dtype=np.float64).reshape(-1, k) for a, k in ((pos, 3), (quat, 4), (vel, 3), (target_pos, 3)))
    tv = np.zeros_like(vel) if target_vel is None else np.asarray(target_vel, dtype=np.float64).reshape(-1, 3)
    acc = K_P * (target_pos - pos) + K_D * (tv - vel) + np.array([0.0, 0.0, G_Z])
    R = _rot(quat)
    thrust = np.sum(acc * R[:, :, 2], axis=-1)
    zb = _unit(acc)
    xb = _unit(np.cross(np.array([0.0, 1.0, 0.0]), zb))
    yb = _unit(np.cross(zb, xb))
    Rt = np.stack([xb, yb, zb], axis=-1)
    Rn = R / np.sum(quat * quat, axis=-1)[:, None, None]         # (the error quaternion scales with |q|: conj(q) (x) q_t is linear in q)
    Re = np.einsum("nji,njk->nik", Rn, Rt)
    vee = np.stack([Re[:, 2, 1] - Re[:, 1, 2], Re[:, 0, 2] - Re[:, 2, 0], Re[:, 1, 0] - Re[:, 0, 1]], axis=-1)
    absw = 0.5 * np.sqrt(np.maximum(1.0 + Re[:, 0, 0] + Re[:, 1, 1] + Re[:, 2, 2], 0.0))
    qn = np.linalg.norm(quat, axis=-1)
    rates = K_RATES * vee / (2.0 * absw[:, None]) * qn[:, None]
    return np.concatenate([thrust[:, None], rates], axis=-1)


def torque_rows(C):
    """[4, 4]: (T, tau_x, tau_y, tau_z) = rows @ f, the integrator's statements (oracle/batched_oracle.py `_substep`, csrc/gpd_common.inc)"""
    kz = (-1.0 if C.DRONE_MODEL == "racer" else 1.0) * C.KM / C.KF
    if C.DRONE_MODEL == "cf2p":
        tx, ty = np.array([0, 1.0, 0, -1.0]) * C.L, np.array([-1.0, 0, 1.0, 0]) * C.L
    else:
        arm = C.L / np.sqrt(2)
        tx, ty = np.array([1.0, 1.0, -1.0, -1.0]) * arm, np.array([-1.0, 1.0, 1.0, -1.0]) * arm
        if C.DRONE_MODEL == "cf2x":
            tx = -tx
    return np.vstack([np.ones(4), tx, ty, kz * np.array([-1.0, 1.0, -1.0, 1.0])])


def rate_loop(C, cmd, w, k_rate=K_RATE, thrust_max=THRUST_MAX, rate_max=RATE_MAX, clipped=None):
    """(b): cmd [n, 4], body rates w [n, 3] -> rpm [n, 4]; `clipped` (a list) receives a bool [n]: some rotor outside [0, f_max]"""
    cmd, w = np.asarray(cmd, dtype=np.float64).reshape(-1, 4), np.asarray(w, dtype=np.float64).reshape(-1, 3)
    thr = np.clip(cmd[:, 0], 0.0, thrust_max)
    wc = np.clip(cmd[:, 1:], -rate_max, rate_max)
    J = np.diag(C.J)
    tau = J * (np.asarray(k_rate) * (wc - w)) + np.cross(w, J * w)
    f = np.linalg.solve(torque_rows(C), np.concatenate([(C.M * thr)[:, None], tau], axis=-1).T).T
    f_max = C.KF * C.MAX_RPM ** 2
    if clipped is not None:
        clipped.append(((f < 0.0) | (f > f_max)).any(axis=-1))
    return np.sqrt(np.clip(f, 0.0, f_max) / C.KF)


class CtbrF64:
    """n single-drone aviaries under the oracle's integrator with the rate loop in every sub-step.  `mass_scale` [n]: the PLANT's mass
    and weight (the controller keeps the nominal M and J), as the per-drone plant table's mass factor."""

    def __init__(self, model="cf2x", n=1, pos=None, quat=None, vel=None, w=None, last_rpm=None, physics_flags=0, pyb_freq=240, ctrl_freq=48,
                 mass_scale=None, **gains):
        self.av = BatchedAviary(URDF[model], drone_model=model, num_envs=n, num_drones=1, physics_flags=physics_flags, pyb_freq=pyb_freq,
                                ctrl_freq=ctrl_freq, act="raw_rpm", initial_xyzs=np.zeros((n, 1, 3)) if pos is None else np.reshape(pos, (n, 1, 3)))
        self.C, self.n, self.gains = self.av.C, n, gains
        self.nominal = UrdfConstants(URDF[model], model)
        for name, v in (("quat", quat), ("vel", vel), ("rpy_rates", w), ("last_rpm", last_rpm)):
            if v is not None:
                setattr(self.av, name, np.asarray(v, dtype=np.float64).reshape(n, 1, -1).copy())
        if mass_scale is not None:
            s = np.asarray(mass_scale, dtype=np.float64).reshape(n, 1)
            self.C.M, self.C.GRAVITY = self.C.M * s[..., None], self.C.GRAVITY * s
        self.clipped_steps, self.steps = np.zeros(n), 0
        self.at_zero, self.at_max = np.zeros(n, dtype=bool), np.zeros(n, dtype=bool)      # a rotor was held at 0 / at f_max

    def step(self, rows, mode="cmd"):
        """one control step; rows [n, 4] commands or [n, 12] / [n, 3] targets -> (obs12 [n, 12], cmd [n, 4])"""
        av = self.av
        rows = np.asarray(rows, dtype=np.float64).reshape(self.n, -1)
        if mode == "pos":
            tv = rows[:, 6:9] if rows.shape[1] == 12 else None
            cmd = outer(av.pos[:, 0], av.quat[:, 0], av.vel[:, 0], rows[:, 0:3], tv)
        else:
            cmd = rows
        hit = np.zeros(self.n, dtype=bool)
        for _ in range(av.S):
            flag = []
            rpm = rate_loop(self.nominal, cmd, av.rpy_rates[:, 0], clipped=flag, **self.gains)[:, None, :]
            hit |= flag[0]
            self.at_zero |= (rpm[:, 0] == 0).any(axis=-1)
            self.at_max |= np.isclose(rpm[:, 0], self.nominal.MAX_RPM, rtol=1e-12, atol=0).any(axis=-1)
            av._substep(rpm, av.last_rpm)
            av.last_rpm = rpm.copy()
        av.rpy = bm.euler_from_quaternion_b(av.quat)
        av.step_counter = av.step_counter + av.S
        self.clipped_steps += hit
        self.steps += 1
        return av.obs12()[:, 0], cmd

    def run(self, rows, K, mode="cmd"):
        """K steps; rows [n, W] held or [K, n, W] -> obs12 [K, n, 12]"""
        rows = np.asarray(rows, dtype=np.float64)
        return np.array([self.step(rows if rows.ndim == 2 else rows[t], mode)[0] for t in range(K)])


def steady_state_error(mass_scale):
    """Where the outer loop -- proportional and derivative terms only -- leaves a drone whose mass is `mass_scale` times the nominal one:
    hovering level needs the thrust command g s, the law gives K_P[2] e_z + g, so e_z = g (s - 1) / K_P[2] below (above) the target."""
    return G_Z * np.abs(np.asarray(mass_scale, dtype=np.float64) - 1.0) / K_P[2]
