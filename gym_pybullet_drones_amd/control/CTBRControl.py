"""`CTBRControl`: the reference's collective-thrust-and-body-rate controller (`control/CTBRControl.py:13-168`, flown by `examples/beta.py`
through `BetaAviary` with Betaflight as the inner loop).

`CTBRControl` is the drop-in single-drone class: numpy float64 on the host, the reference's signatures and its 4-tuple
`(thrust [m/s^2], rate_x, rate_y, rate_z [rad/s])`.  It is thirty floating-point operations per call, so it launches nothing.
`VectorCTBR` runs n of them per call on torch tensors (`gpd_ctbr`, include/gpd.h) and carries what `SimCore.rollout_ctbr` needs on top:
the gains, clips and rotor allocation of the body-rate loop that stands in for the firmware (`struct GpdCtbr`, csrc/ctbr_math.inc,
DESIGN.md section 3.17).
"""
import numpy as np
import torch

from .. import _native
from ..engine import as_f32, resolve_device
from ..params import DroneParams
from ..utils.enums import DroneModel
from .BaseControl import BaseControl

#: the constants of the reference's method (`:149-152`)
G_Z, K_P, K_D, K_RATES = 9.8, (3.0, 3.0, 8.0), (2.5, 2.5, 5.0), (5.0, 5.0, 1.0)
#: the rate loop's defaults: gains [1/s], and `BetaAviary.ctbr2beta`'s command limits (`envs/BetaAviary.py:176-188`): 40.9 m/s^2, 360 deg/s
K_RATE, THRUST_MAX, RATE_MAX = (40.0, 40.0, 20.0), 40.9, 2.0 * np.pi
_MODELS = (DroneModel.CF2X, DroneModel.CF2P, DroneModel.RACE)


def _unit(v):
    return v / np.sqrt(np.sum(v * v))


def quat_from_matrix(m: np.ndarray) -> np.ndarray:
    """(w, x, y, z) of a rotation matrix, Shepperd's four cases; the sign is whatever the case gives (the caller does not depend on it)"""
    tr = m[0, 0] + m[1, 1] + m[2, 2]
    if tr > 0:
        s = 2.0 * np.sqrt(1.0 + tr)
        return np.array([0.25 * s, (m[2, 1] - m[1, 2]) / s, (m[0, 2] - m[2, 0]) / s, (m[1, 0] - m[0, 1]) / s])
    if m[0, 0] > m[1, 1] and m[0, 0] > m[2, 2]:
        s = 2.0 * np.sqrt(1.0 + m[0, 0] - m[1, 1] - m[2, 2])
        return np.array([(m[2, 1] - m[1, 2]) / s, 0.25 * s, (m[0, 1] + m[1, 0]) / s, (m[0, 2] + m[2, 0]) / s])
    if m[1, 1] > m[2, 2]:
        s = 2.0 * np.sqrt(1.0 + m[1, 1] - m[0, 0] - m[2, 2])
        return np.array([(m[0, 2] - m[2, 0]) / s, (m[0, 1] + m[1, 0]) / s, 0.25 * s, (m[1, 2] + m[2, 1]) / s])
    s = 2.0 * np.sqrt(1.0 + m[2, 2] - m[0, 0] - m[1, 1])
    return np.array([(m[1, 0] - m[0, 1]) / s, (m[0, 2] + m[2, 0]) / s, (m[1, 2] + m[2, 1]) / s, 0.25 * s])


def _qmult(a, b):
    """Hamilton product, (w, x, y, z)"""
    return np.array([a[0] * b[0] - a[1] * b[1] - a[2] * b[2] - a[3] * b[3], a[0] * b[1] + a[1] * b[0] + a[2] * b[3] - a[3] * b[2],
                     a[0] * b[2] - a[1] * b[3] + a[2] * b[0] + a[3] * b[1], a[0] * b[3] + a[1] * b[2] - a[2] * b[1] + a[3] * b[0]])


def allocation(P: DroneParams) -> np.ndarray:
    """[4, 3] float64: f = M thrust / 4 + alloc @ tau, the exact inverse of the integrator's torque rows (csrc/gpd_common.inc, `substep`)
    for the airframe.  The four rows (total thrust and three torques as functions of the rotor thrusts) are mutually orthogonal, so the
    inverse is the transpose with each row divided by its squared norm."""
    kz = (-1.0 if P.DRONE_MODEL == DroneModel.RACE else 1.0) * P.KM / P.KF
    if P.DRONE_MODEL == DroneModel.CF2P:
        rows = np.array([[0.0, 1.0, 0.0, -1.0], [-1.0, 0.0, 1.0, 0.0]]) * P.L
    else:
        arm = P.L / np.sqrt(2.0)
        rows = np.array([[1.0, 1.0, -1.0, -1.0], [-1.0, 1.0, 1.0, -1.0]]) * arm
        if P.DRONE_MODEL == DroneModel.CF2X:
            rows[0] = -rows[0]
    rows = np.vstack([rows, kz * np.array([-1.0, 1.0, -1.0, 1.0])])
    return (rows / np.sum(rows * rows, axis=1, keepdims=True)).T


def to_struct(P: DroneParams, k_rate=K_RATE, thrust_max: float = THRUST_MAX, rate_max: float = RATE_MAX) -> "_native.GpdCtbr":
    """`struct GpdCtbr` for the airframe: the reference's outer-loop constants, the rate loop's gains and clips, the allocation and the
    rotor limits rounded once from float64.  ValueError for gains or clips that are not finite and positive."""
    k_rate = np.asarray(k_rate, dtype=np.float64).reshape(-1)
    if k_rate.shape != (3,) or not np.all(np.isfinite(k_rate)) or not np.all(k_rate > 0):
        raise ValueError("CTBR: k_rate must be three finite positive gains [1/s]")
    for name, v in (("thrust_max", thrust_max), ("rate_max", rate_max)):
        if not (np.isfinite(v) and v > 0):
            raise ValueError(f"CTBR: {name} must be finite and positive")
    s = _native.GpdCtbr()
    for i in range(3):
        s.k_p[i], s.k_d[i], s.k_rates[i], s.k_rate[i] = K_P[i], K_D[i], K_RATES[i], k_rate[i]
    s.g, s.thrust_max, s.rate_max = G_Z, float(thrust_max), float(rate_max)
    for i, v in enumerate(allocation(P).reshape(-1)):
        s.alloc[i] = v
    s.f_max, s.inv_kf = P.KF * P.MAX_RPM ** 2, 1.0 / P.KF
    return s


class CTBRControl(BaseControl):
    """Control class for thrust and body-rate commands -- single drone, numpy interface of the reference."""

    def __init__(self, drone_model: DroneModel, g: float = 9.8):
        super().__init__(drone_model=drone_model, g=g)

    def computeControlFromState(self, control_timestep, state, target_pos, target_rpy=np.zeros(3), target_vel=np.zeros(3),
                                target_rpy_rates=np.zeros(3)):
        """`computeControl` fed from a (20,) state vector; the quaternion is reordered to (w, x, y, z) as the reference does (`:92`)."""
        return self.computeControl(control_timestep=control_timestep, cur_pos=state[0:3],
                                   cur_quat=np.array([state[6], state[3], state[4], state[5]]), cur_vel=state[10:13],
                                   cur_ang_vel=state[13:16], target_pos=target_pos, target_rpy=target_rpy, target_vel=target_vel,
                                   target_rpy_rates=target_rpy_rates)

    def computeControl(self, control_timestep, cur_pos, cur_quat, cur_vel, cur_ang_vel, target_pos, target_rpy=np.zeros(3),
                       target_vel=np.zeros(3), target_rpy_rates=np.zeros(3)):
        """-> (thrust [m/s^2], rate_x, rate_y, rate_z [rad/s]).  `cur_quat` is (w, x, y, z) HERE (the reference's quirk: its
        `computeControlFromState` reorders the state's x, y, z, w).  `target_rpy` and `target_rpy_rates` are accepted and ignored, and the
        gravity of the law is the method's own 9.8, not the constructor's `g` -- both as in the reference (`:149-168`)."""
        for name, v, k in (("cur_pos", cur_pos, 3), ("cur_quat", cur_quat, 4), ("cur_vel", cur_vel, 3), ("cur_ang_vel", cur_ang_vel, 3),
                           ("target_pos", target_pos, 3), ("target_rpy", target_rpy, 3), ("target_vel", target_vel, 3),
                           ("target_rpy_rates", target_rpy_rates, 3)):
            assert np.shape(v) == (k,), f"{name} {np.shape(v)}"
        q = np.asarray(cur_quat, dtype=np.float64)
        tar_acc = (np.array(K_P) * (np.asarray(target_pos, dtype=np.float64) - cur_pos)
                   + np.array(K_D) * (np.asarray(target_vel, dtype=np.float64) - cur_vel) + np.array([0.0, 0.0, G_Z]))
        w, x, y, z = q
        z_world = np.array([2.0 * (x * z + w * y), 2.0 * (y * z - w * x), w * w - x * x - y * y + z * z])        # q (0, 0, 1) q*
        norm_thrust = float(np.dot(tar_acc, z_world))
        z_body = _unit(tar_acc)
        x_body = _unit(np.cross(np.array([0.0, 1.0, 0.0]), z_body))
        y_body = _unit(np.cross(z_body, x_body))
        tar_att = quat_from_matrix(np.vstack([x_body, y_body, z_body]).T)
        q_error = _qmult(np.array([w, -x, -y, -z]), tar_att)
        body_rates = 2.0 * np.array(K_RATES) * q_error[1:]
        if q_error[0] < 0:
            body_rates = -body_rates
        return (norm_thrust, *body_rates)


class VectorCTBR(BaseControl):
    """n independent CTBR controllers, one lane each (`gpd_ctbr`), and the rate loop's constants for `SimCore.rollout_ctbr`."""

    def __init__(self, num: int, drone_model: DroneModel = DroneModel.CF2X, device=None, k_rate=K_RATE, thrust_max: float = THRUST_MAX,
                 rate_max: float = RATE_MAX, g: float = 9.8):
        if drone_model not in _MODELS:
            raise ValueError("VectorCTBR requires DroneModel.CF2X, DroneModel.CF2P or DroneModel.RACE")
        self.n = int(num)
        if self.n < 1:
            raise ValueError("VectorCTBR: num must be >= 1")
        super().__init__(drone_model=drone_model, g=g)
        self._struct = to_struct(self._drone_params, k_rate, thrust_max, rate_max)
        self.k_rate, self.thrust_max, self.rate_max = tuple(float(v) for v in np.reshape(k_rate, -1)), float(thrust_max), float(rate_max)
        self.lib = _native.lib()
        self.device = resolve_device(device, "VectorCTBR")

    def struct(self) -> "_native.GpdCtbr":
        return self._struct

    def compute(self, pos, quat, vel, target_pos, target_vel=None) -> torch.Tensor:
        """Batched outer loop -> `cmd [n, 4]` (thrust [m/s^2] | body rates [rad/s]), a float32 device tensor.  `quat` is x, y, z, w -- the
        state's order (`SimCore.quaternions()`).  Asynchronous on the current stream, capturable in a hipGraph when every input is a
        contiguous float32 device tensor already."""
        n, dev = self.n, self.device
        for name, x, k in (("pos", pos, 3), ("quat", quat, 4), ("vel", vel, 3), ("target_pos", target_pos, 3), ("target_vel", target_vel, 3)):
            if x is not None and int(np.prod(np.shape(x))) != n * k:
                raise ValueError(f"VectorCTBR.compute: {name} must hold {n} x {k} values, got shape {tuple(np.shape(x))}")
        a = [as_f32(x, n, k, dev) for x, k in ((pos, 3), (quat, 4), (vel, 3), (target_pos, 3), (target_vel, 3))]
        cmd = torch.empty((n, 4), dtype=torch.float32, device=dev)
        _native.call("gpd_ctbr", dev, _native.raw_stream(dev), self._struct, *a, cmd, n)
        self.control_counter += 1
        return cmd

    def rotor_forces(self, cmd: torch.Tensor, body_rates: torch.Tensor) -> torch.Tensor:
        """The rate loop's steps 1-4 as torch operations -> the UNCLIPPED rotor thrusts `f [n, 4]` [N] for commands `cmd [n, 4]` and body
        rates `[n, 3]`: a diagnostic (is a rotor outside `[0, f_max]`?) and the per-sub-step restatement profiles/ctbr_bench.py times
        the fused kernel against.  `rollout_ctbr` does not come through here."""
        s, P = self._struct, self._drone_params
        if getattr(self, "_torch_consts", None) is None or self._torch_consts[0].device != cmd.device:       # (built once: no copies per call)
            f32 = lambda v: torch.tensor(np.asarray(v, dtype=np.float32), device=cmd.device)      # noqa: E731
            self._torch_consts = (f32(np.diag(P.J)), f32(list(s.k_rate)), f32(list(s.alloc)).view(4, 3))
        J, k, alloc = self._torch_consts
        thr = cmd[:, 0].clamp(0.0, s.thrust_max)
        wc = cmd[:, 1:4].clamp(-s.rate_max, s.rate_max)
        tau = J * (k * (wc - body_rates)) + torch.linalg.cross(body_rates, J * body_rates)
        return (0.25 * float(P.M)) * thr.unsqueeze(1) + tau @ alloc.t()

    @property
    def f_max(self) -> float:
        """a rotor's largest thrust [N], KF MAX_RPM^2"""
        return float(self._struct.f_max)
