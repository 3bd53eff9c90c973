"""`MRAC`: the reference's model-reference adaptive controller (`control/MRAC.py:12-155`, flown by `examples/mrac.py`) on the GPU.

`MRAC` is the drop-in single-drone class (numpy in / numpy out, the reference's signature and `(rpm, pos_e, rpy_e)` return);
`VectorMRAC` runs n independent controllers per call on torch tensors and is what `SimCore.rollout_mrac` carries through a fused
rollout.  Both call `gpd_mrac` (include/gpd.h) -- the same device function `gpd_rollout_mrac` evaluates between two env steps.

The DESIGN (`_compute_K`, `:56-104`: pole placement, the Lyapunov equation) runs on the host in float64 at construction.  The
reference calls python-control's `place`, which IS `scipy.signal.place_poles(A, B, poles, method="YT").gain_matrix`; scipy is
imported lazily, here only: the rest of the package imports without it.

Controller state per controller: 76 floats `[76][ld]` -- Kx (12 x 4) | Kr (4 x 4) | Xm (12) -- and an int32 call counter.
"""
import numpy as np
import torch

from .. import _native
from ..engine import as_f32, resolve_device, zeros
from ..params import MIXER
from ..utils.enums import DroneModel
from .BaseControl import BaseControl

#: the reference's constants (`:30-33`, `:142`)
PWM2RPM_SCALE, PWM2RPM_CONST, MIN_PWM, MAX_PWM, MAX_TORQUE = 0.2685, 4070.3, 20000, 65535, 3200.0
_MODELS = (DroneModel.CF2X, DroneModel.CF2P, DroneModel.RACE)


def mixer_matrix(drone_model: DroneModel) -> np.ndarray:
    """`:37-50`: RACE flies the CF2X mixer"""
    return MIXER[DroneModel.CF2P if drone_model == DroneModel.CF2P else DroneModel.CF2X].copy()


def design(mass: float, ixx: float, iyy: float, izz: float, g: float = 9.8, psi: float = 0.0) -> dict:
    """`MRAC._compute_K` (`:56-104`) in float64: A, B, K (poles -1 .. -12), Kr_ref_gain, Am, Bm, P, and the initial gains."""
    from scipy.linalg import solve_continuous_lyapunov       # (`solve_lyapunov`, `:6`, is this function's former name)
    from scipy.signal import place_poles
    a_sub = np.array([[0, 0, 0, g * np.sin(psi), g * np.cos(psi), 0],
                      [0, 0, 0, -g * np.cos(psi), g * np.sin(psi), 0]])
    a_sub = np.vstack((a_sub, np.zeros((4, 6))))
    A = np.block([[np.zeros((6, 6)), np.eye(6)], [a_sub, np.zeros((6, 6))]])
    b_sub = np.diag([1 / mass, 1 / ixx, 1 / iyy, 1 / izz])
    B = np.vstack((np.zeros((8, 4)), b_sub))
    Q = np.eye(12) * 600
    K = place_poles(A, B, -np.linspace(1, 12, 12), method="YT").gain_matrix
    Kr_ref_gain = np.linalg.pinv(B) @ (A - B @ K)
    Am = A - B @ K
    Bm = np.copy(B)
    P = solve_continuous_lyapunov(Am.T, -Q)
    return {"A": A, "B": B, "K": K, "Kr_ref_gain": Kr_ref_gain, "Am": Am, "Bm": Bm, "P": P, "Kx0": -K.T, "Kr0": np.eye(4)}


def to_struct(d: dict, gamma_x: float, gamma_r: float, mixer: np.ndarray, kf: float) -> "_native.GpdMrac":
    """The design as the fp32 constants of `struct GpdMrac`, rounded once from float64.  Am / Bm travel in the compact form their
    structure allows (include/gpd.h); a design without that structure is refused rather than truncated."""
    Am, Bm = d["Am"], d["Bm"]
    top = np.zeros((8, 12))
    top[:6, 6:] = np.eye(6)
    top[6:8, 3:5] = Am[6:8, 3:5]
    if not (np.array_equal(Am[:8], top) and np.array_equal(Bm[:8], np.zeros((8, 4))) and np.array_equal(Bm[8:], np.diag(np.diag(Bm[8:])))):
        raise ValueError("MRAC: Am / Bm do not have the structure of the reference's design (include/gpd.h, GpdMrac)")
    s = _native.GpdMrac()

    def fill(dst, src):
        for i, v in enumerate(np.asarray(src, dtype=np.float64).reshape(-1)):
            dst[i] = v
    fill(s.PB, d["P"] @ Bm)
    fill(s.Kr_ref_gain, d["Kr_ref_gain"])
    fill(s.Am_lo, Am[8:])
    fill(s.A_grav, Am[6:8, 3:5])
    fill(s.B_diag, np.diag(Bm[8:]))
    fill(s.mixer, mixer)
    s.gamma_x, s.gamma_r = gamma_x, gamma_r
    s.inv_4kf, s.max_torque = 1.0 / (4.0 * kf), MAX_TORQUE
    s.pwm2rpm_scale, s.inv_pwm2rpm_scale, s.pwm2rpm_const = PWM2RPM_SCALE, 1.0 / PWM2RPM_SCALE, PWM2RPM_CONST
    s.min_pwm, s.max_pwm = MIN_PWM, MAX_PWM
    fill(s.Kx0, d["Kx0"])
    fill(s.Kr0, d["Kr0"])
    return s


def _scalar_of_identity(value, n: int, name: str) -> float:
    m = np.asarray(value, dtype=np.float64)
    if m.shape == ():
        return float(m)
    if m.shape != (n, n) or not np.array_equal(m, np.eye(n) * m[0, 0]):
        raise ValueError(f"MRAC: {name} must be a multiple of the {n} x {n} identity (the device carries one scalar)")
    return float(m[0, 0])


class VectorMRAC(BaseControl):
    """n independent MRAC controllers, one lane each; state `[76][ld]` + counters in device memory."""

    def __init__(self, num: int, drone_model: DroneModel = DroneModel.CF2X, device=None, gamma: float = 5e-3, g: float = 9.8,
                 host_visible: bool = False):
        if drone_model not in _MODELS:
            raise ValueError("[ERROR] MRAC requires DroneModel.CF2X or DroneModel.CF2P or DroneModel.RACE")
        self.lib = _native.lib()
        self.device = resolve_device(device, "MRAC")
        self.n = int(num)
        if self.n < 1:
            raise ValueError("VectorMRAC: num must be >= 1")
        self.ld = (self.n + 63) // 64 * 64
        self.host_visible = bool(host_visible)
        self.state = zeros((_native.MRAC_STATE, self.ld), torch.float32, self.device, self.host_visible)
        self.counter = zeros((self.ld,), torch.int32, self.device, self.host_visible)
        super().__init__(drone_model=drone_model, g=g)
        self.Ixx, self.Iyy, self.Izz = (self._getURDFParameter(k) for k in ("ixx", "iyy", "izz"))
        self.J = np.diag([self.Ixx, self.Iyy, self.Izz])
        self.mass, self.l, self.g = self._getURDFParameter("m"), self._getURDFParameter("arm"), g
        self.PWM2RPM_SCALE, self.PWM2RPM_CONST, self.MIN_PWM, self.MAX_PWM = PWM2RPM_SCALE, PWM2RPM_CONST, MIN_PWM, MAX_PWM
        self.Ka, self.Km = self.KF, self.KM
        self.MIXER_MATRIX = mixer_matrix(drone_model)
        self._design = design(self.mass, self.Ixx, self.Iyy, self.Izz, g)
        self.Am, self.Bm, self.P, self.Kr_ref_gain = (self._design[k] for k in ("Am", "Bm", "P", "Kr_ref_gain"))
        self._gamma = [float(gamma), float(gamma)]
        self._struct = None
        self.reset(gains=True)

    # ---- the design's constants ---------------------------------------------------------------------------------------------
    def struct(self) -> "_native.GpdMrac":
        if self._struct is None:
            self._struct = to_struct(self._design, self._gamma[0], self._gamma[1], self.MIXER_MATRIX, self.KF)
        return self._struct

    Gamma_x = property(lambda self: np.eye(12) * self._gamma[0])
    Gamma_r = property(lambda self: np.eye(4) * self._gamma[1])

    @Gamma_x.setter
    def Gamma_x(self, value):
        self._gamma[0], self._struct = _scalar_of_identity(value, 12, "Gamma_x"), None

    @Gamma_r.setter
    def Gamma_r(self, value):
        self._gamma[1], self._struct = _scalar_of_identity(value, 4, "Gamma_r"), None

    # ---- BaseControl surface ------------------------------------------------------------------------------------------------
    def reset(self, mask=None, gains: bool = False):
        """The reference's `reset()` (`:106-107`): the call counters (of the controllers in the bool/uint8 `mask` [n]; None: all) go
        to zero and nothing else -- the next call re-seeds Xm from the state it sees, the ADAPTED GAINS SURVIVE.  `gains=True` (an
        extra) also restores the design's Kx0 / Kr0."""
        if not hasattr(self, "_design"):        # (BaseControl.__init__ resets before the design exists: the buffers are zero)
            return
        if mask is not None:
            mask = torch.as_tensor(mask).to(device=self.device, dtype=torch.uint8).contiguous()
            if mask.numel() != self.n:
                raise ValueError(f"VectorMRAC.reset: mask has {mask.numel()} elements, expected {self.n}")
        _native.call("gpd_mrac_reset", self.device, _native.raw_stream(self.device), self.state, self.counter, self.ld, self.struct(), mask,
                     self.n, int(bool(gains)))

    @property
    def control_counter(self):
        """[n] int32 device tensor: calls since the controller's last reset"""
        return self.counter[:self.n]

    @control_counter.setter
    def control_counter(self, value):      # (BaseControl.reset assigns 0)
        self.counter.fill_(int(value))

    def gains(self):
        """`(Kx [12, 4, n], Kr [4, 4, n])` VIEWS of the adapted gains"""
        return self.state[:48, :self.n].view(12, 4, self.n), self.state[48:64, :self.n].view(4, 4, self.n)

    def model_state(self) -> torch.Tensor:
        """`Xm [12, n]` VIEW of the reference model's state"""
        return self.state[64:76, :self.n]

    def get_state(self) -> dict:
        """Snapshot (clones) of everything a later call depends on; `set_state(**get_state())` resumes bit for bit."""
        return {"state": self.state[:, :self.n].clone(), "counter": self.counter[:self.n].clone()}

    def set_state(self, state=None, counter=None):
        for dst, src in ((self.state[:, :self.n], state), (self.counter[:self.n], counter)):
            if src is not None:
                src = torch.as_tensor(src, device=dst.device)
                if tuple(src.shape) != tuple(dst.shape):
                    raise ValueError(f"VectorMRAC.set_state: shape {tuple(src.shape)}, expected {tuple(dst.shape)}")
                dst.copy_(src.to(dst.dtype))

    def compute(self, control_timestep, cur_pos, cur_quat, cur_vel, cur_ang_vel, target_pos, target_rpy=None, target_vel=None,
                target_rpy_rates=None):
        """Batched `computeControl` -> `(rpm [n, 4], pos_e [n, 3], rpy_e [n, 3])` float32 device tensors; asynchronous on the
        current stream, capturable in a hipGraph when every input is a contiguous float32 device tensor already."""
        n, dev = self.n, self.device
        a = [as_f32(x, n, k, dev) for x, k in ((cur_pos, 3), (cur_quat, 4), (cur_vel, 3), (cur_ang_vel, 3), (target_pos, 3), (target_rpy, 3),
                                          (target_vel, 3), (target_rpy_rates, 3))]
        rpm = torch.empty((n, 4), dtype=torch.float32, device=dev)
        pos_e = torch.empty((n, 3), dtype=torch.float32, device=dev)
        rpy_e = torch.empty((n, 3), dtype=torch.float32, device=dev)
        _native.call("gpd_mrac", dev, _native.raw_stream(dev), self.struct(), self.state, self.counter, self.ld, float(control_timestep), *a,
                     rpm, pos_e, rpy_e, n)
        return rpm, pos_e, rpy_e

    computeControl = compute


class MRAC(VectorMRAC):
    """Model Reference Adaptive Controller class for Crazyflies -- single drone, numpy interface of the reference.  State, counter
    and the call's operands live in page-locked host memory the device addresses directly: a call is one `gpd_mrac` launch and one
    wait for the stream, no copies."""

    # one page-locked block for the call's operands, float offsets (the two 16-byte accesses of gpd_mrac_kernel first)
    _QUAT, _RPM, _POS, _VEL, _ANGV, _TPOS, _TRPY, _TVEL, _TRATES, _POS_E, _RPY_E, _IO_FLOATS = 0, 4, 8, 11, 14, 17, 20, 23, 26, 29, 32, 36

    def __init__(self, drone_model: DroneModel, g: float = 9.8, device=None):
        if drone_model not in _MODELS:
            print("[ERROR] MRAC requires DroneModel.CF2X or DroneModel.CF2P or DroneModel.RACE")
            exit()
        super().__init__(1, drone_model=drone_model, device=device, g=g, host_visible=True)
        self._io_t = zeros((self._IO_FLOATS,), torch.float32, self.device, host_visible=True)
        self._io = self._io_t.numpy()
        at = lambda off: _native.as_c(self._io_t[off:])      # noqa: E731
        self._args = [_native.as_c(self.state), _native.as_c(self.counter)] + [at(o) for o in (self._POS, self._QUAT, self._VEL, self._ANGV, self._TPOS, self._TRPY, self._TVEL, self._TRATES,
                                      self._RPM, self._POS_E, self._RPY_E)]

    def _wait(self):
        torch.cuda.current_stream(self.device).synchronize()

    def reset(self, gains: bool = False):
        super().reset(gains=gains)
        if hasattr(self, "_design"):
            self._wait()

    # the reference's members, read back from the controller's state
    @property
    def control_counter(self):
        self._wait()
        return int(self.counter[0])

    @control_counter.setter
    def control_counter(self, value):
        self._wait()
        self.counter[0] = int(value)

    @property
    def Kx(self):
        self._wait()
        return self.state[:48, 0].numpy().astype(np.float64).reshape(12, 4)

    @property
    def Kr(self):
        self._wait()
        return self.state[48:64, 0].numpy().astype(np.float64).reshape(4, 4)

    @property
    def Xm(self):
        self._wait()
        return self.state[64:76, 0].numpy().astype(np.float64).reshape(12, 1)

    def computeControl(self, control_timestep, cur_pos, cur_quat, cur_vel, cur_ang_vel, target_pos, target_rpy=np.zeros(3),
                       target_vel=np.zeros(3), target_rpy_rates=np.zeros(3)):
        """-> (rpm (4,), pos_e (3,), rpy_e (3,)), float64 numpy like the reference."""
        io = self._io
        for off, v, k in ((self._QUAT, cur_quat, 4), (self._POS, cur_pos, 3), (self._VEL, cur_vel, 3), (self._ANGV, cur_ang_vel, 3),
                          (self._TPOS, target_pos, 3), (self._TRPY, target_rpy, 3), (self._TVEL, target_vel, 3),
                          (self._TRATES, target_rpy_rates, 3)):
            io[off:off + k] = v
        a = self._args
        with _native.device_guard(self.device):
            rc = self.lib.gpd_mrac(_native.as_c(self.struct()), a[0], a[1], self.ld, float(control_timestep),
                                   a[2], a[3], a[4], a[5], a[6], a[7], a[8], a[9], a[10], a[11], a[12], 1, _native.raw_stream(self.device))
        if rc:
            _native.check(rc, "gpd_mrac")
        self._wait()
        out = io.astype(np.float64)
        return out[self._RPM:self._RPM + 4], out[self._POS_E:self._POS_E + 3], out[self._RPY_E:self._RPY_E + 3]
