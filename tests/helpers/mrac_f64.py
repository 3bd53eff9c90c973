"""Float64 restatement of the reference's `MRAC.computeControl` (`control/MRAC.py:109-155`), statement by statement, without
pybullet, scipy's `Rotation` or python-control: the yardstick the device's fp32 controller is measured against, itself checked
against the recorded calls of the reference (tests/test_host_mrac.py)."""
import numpy as np

PWM2RPM_SCALE, PWM2RPM_CONST, MIN_PWM, MAX_PWM = 0.2685, 4070.3, 20000, 65535


def euler_from_quaternion(q):
    """pybullet's getEulerFromQuaternion (Bullet's btMatrix3x3::getEulerZYX on the quaternion's squares), gimbal branches included"""
    x, y, z, w = (float(v) for v in q)
    sqx, sqy, sqz, squ = x * x, y * y, z * z, w * w
    sarg = -2.0 * (x * z - w * y)
    if sarg <= -0.99999:
        return np.array([0.0, -0.5 * np.pi, 2 * np.arctan2(x, -y)])
    if sarg >= 0.99999:
        return np.array([0.0, 0.5 * np.pi, 2 * np.arctan2(-x, y)])
    return np.array([np.arctan2(2 * (y * z + w * x), squ - sqx - sqy + sqz), np.arcsin(sarg),
                     np.arctan2(2 * (x * y + w * z), squ + sqx - sqy - sqz)])


def intrinsic_xyz(rpy):
    """scipy's Rotation.from_euler('XYZ', rpy).as_matrix(): R = Rx(roll) Ry(pitch) Rz(yaw)"""
    cr, sr, cp, sp, cy, sy = np.cos(rpy[0]), np.sin(rpy[0]), np.cos(rpy[1]), np.sin(rpy[1]), np.cos(rpy[2]), np.sin(rpy[2])
    Rx = np.array([[1, 0, 0], [0, cr, -sr], [0, sr, cr]])
    Ry = np.array([[cp, 0, sp], [0, 1, 0], [-sp, 0, cp]])
    Rz = np.array([[cy, -sy, 0], [sy, cy, 0], [0, 0, 1]])
    return Rx @ Ry @ Rz


class MracF64:
    """The reference class's members and its one method, in float64.  `design`: an `mrac_design_<m>.npz` mapping."""

    def __init__(self, design, gamma=None):
        g = float(design["gamma"]) if gamma is None else gamma
        self.Am, self.Bm, self.P, self.Kr_ref_gain = (np.array(design[k], dtype=np.float64) for k in ("Am", "Bm", "P", "Kr_ref_gain"))
        self.Gamma_x, self.Gamma_r = np.eye(12) * g, np.eye(4) * g
        self.MIXER_MATRIX, self.KF = np.array(design["mixer"], dtype=np.float64), float(design["KF"])
        self.Kx, self.Kr = np.array(design["Kx0"], dtype=np.float64), np.array(design["Kr0"], dtype=np.float64)
        self.Xm = np.zeros((12, 1))
        self.control_counter = 0

    def computeControl(self, control_timestep, cur_pos, cur_quat, cur_vel, cur_ang_vel, target_pos, target_rpy=np.zeros(3),
                       target_vel=np.zeros(3), target_rpy_rates=np.zeros(3)):
        cur_rpy = euler_from_quaternion(cur_quat)
        cur_ang_vel = intrinsic_xyz(cur_rpy).T @ np.asarray(cur_ang_vel, dtype=np.float64)       # .inv().apply()
        if self.control_counter == 0:
            self.Xm = np.hstack((cur_pos, cur_rpy, cur_vel, cur_ang_vel)).reshape(12, 1)
        self.control_counter += 1
        r = np.hstack((target_pos, target_rpy, target_vel, target_rpy_rates)).reshape(12, 1)
        rt = -self.Kr_ref_gain @ r
        X_actual = np.hstack((cur_pos, cur_rpy, cur_vel, cur_ang_vel)).reshape(12, 1)
        u = self.Kx.T @ X_actual + self.Kr.T @ rt
        e = X_actual - self.Xm
        Kx_dot = -self.Gamma_x @ X_actual @ e.T @ self.P @ self.Bm
        Kr_dot = -self.Gamma_r @ rt @ e.T @ self.P @ self.Bm
        self.Kx = self.Kx + Kx_dot * control_timestep
        self.Kr = self.Kr + Kr_dot * control_timestep
        thrust, tx, ty, tz = u.squeeze()
        thrust = np.maximum(0, thrust)
        target_torques = np.clip(np.hstack((tx, ty, tz)), -3200, 3200)
        thrust = (np.sqrt(thrust / (4 * self.KF)) - PWM2RPM_CONST) / PWM2RPM_SCALE
        pwm = np.clip(thrust + np.dot(self.MIXER_MATRIX, target_torques), MIN_PWM, MAX_PWM)
        rpm = PWM2RPM_SCALE * pwm + PWM2RPM_CONST
        pos_e = np.asarray(target_pos, dtype=np.float64) - cur_pos
        rpy_e = np.asarray(target_rpy, dtype=np.float64) - cur_rpy
        Xm_dot = self.Am @ self.Xm + self.Bm @ rt
        self.Xm = self.Xm + Xm_dot * control_timestep
        return rpm, pos_e, rpy_e


def rel_err(x, ref):
    """the project's metric: max|x - ref| / max(max|ref|, 1)"""
    x, ref = np.asarray(x, dtype=np.float64), np.asarray(ref, dtype=np.float64)
    return float(np.max(np.abs(x - ref)) / max(float(np.max(np.abs(ref))), 1.0))
