"""The differentiable rollout on thrust and body-rate commands, without a GPU:
  1. the yardstick tests/helpers/diff_ctbr_f64.py: its forward against tests/helpers/ctbr_f64.py's closed loop (1e-12), its gradients
     under torch.autograd.gradcheck, the populations on both sides of every select its input kinds exist for, the float32 run of the
     restatement taking the same branch as the float64 one at every evaluation of every select, and float32 gradients within 1e-5 of
     the float64 ones (DESIGN.md section 3.12's rule for a reference that fp32 kernels are held against);
  2. csrc/ctbr_vjp.inc -- the text the device sweep compiles -- evaluated in fp32 by the stand-alone program tests/c/diff_ctbr_host.c
     (ASan + UBSan) on 4 096 seeded inputs per airframe and kind, against float64 autograd: max |g32 - g64| / max |g64| per output group
     <= 1e-4; the same program holds the adjoint text against the forward text (<v, J u> = <J^T v, u>) and drives the entries' host side;
  3. the binding, the tape's size and the refusals of the three entries through ctypes, one broken argument at a time, and the Python
     layer's refusals before any device work."""
import ctypes
import os
import struct
import sys
import types

import numpy as np
import pytest
import torch

from conftest import REPO

sys.path.insert(0, os.path.join(REPO, "tests", "helpers"))
import ctbr_f64 as H  # noqa: E402
import diff_ctbr_f64 as D  # noqa: E402
import host_lib  # noqa: E402

MODELS = ("cf2x", "cf2p", "racer")
TOL = 1e-4          # the project's limit, here in the gradient tests' metric max |g32 - g64| / max |g64|
F32_RULE = 1e-5     # the restatement's own float32 gradients against its float64 ones


def _model(name):
    from gym_pybullet_drones_amd.utils.enums import DroneModel
    return DroneModel(name)


# ---- 1. the yardstick ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("model,S,mode", [("cf2x", 5, "cmd"), ("cf2p", 8, "pos"), ("racer", 1, "pos"), ("cf2x", 5, "pos")])
def test_forward_equals_the_ctbr_yardstick(model, S, mode):
    """obs12 of 4 steps equals tests/helpers/ctbr_f64.py's closed loop (its own outer loop on rotation matrices, its rate loop through
    the square root, the oracle's integrator) to 1e-12, with rare lanes of every kind of the mode among the drones; a population of
    masses too"""
    C = H.UrdfConstants(H.URDF[model], model)
    for kind in ("plain",) + (D.CMD_KINDS if mode == "cmd" else D.POS_KINDS):
        for mass in (None, np.linspace(0.8, 1.2, 12)):
            inp = D.make_inputs(C, 12, 4, mode, kind, seed=5)
            if kind != "plain":          # (12 drones: the rare lanes are drones 0, 3, 6, 9)
                assert inp.rare.sum() == 4
            sim = H.CtbrF64(model, 12, pos=inp.pos, quat=inp.quat, vel=inp.vel, w=inp.rates, ctrl_freq=240 // S, mass_scale=mass)
            want = sim.run(inp.rows, 4, mode)
            scales = None if mass is None else np.vstack([mass, np.ones((8, 12))])
            T = lambda v: torch.as_tensor(v, dtype=torch.float64)     # noqa: E731
            got, _ = D.rollout(D.consts(C, 12, scales=scales), D.controller(C), D.config(model, S), T(D.GAINS),
                               tuple(T(v) for v in (inp.pos, inp.quat, inp.vel, inp.rates)), T(inp.rows), mode)
            err = float(np.abs(got.numpy() - want).max() / max(1.0, np.abs(want).max()))
            assert err < 1e-12, (model, mode, kind, err)


@pytest.mark.parametrize("mode", ["cmd", "pos"])
def test_gradients_pass_gradcheck(mode):
    C = H.UrdfConstants(H.URDF["cf2x"], "cf2x")
    inp = D.make_inputs(C, 2, 2, mode, seed=7)
    c, ctl, cfg = D.consts(C, 2), D.controller(C), D.config("cf2x", 2)
    leaf = lambda v: torch.tensor(v, dtype=torch.float64, requires_grad=True)     # noqa: E731

    def f(rows, pos, quat, vel, rates, gains):
        obs, kin = D.rollout(c, ctl, cfg, gains, (pos, quat, vel, rates), rows, mode)
        return (obs,) + tuple(kin)
    assert torch.autograd.gradcheck(f, tuple(leaf(v) for v in (inp.rows, inp.pos, inp.quat, inp.vel, inp.rates, D.GAINS)), eps=1e-6, atol=1e-6, rtol=1e-5)


_RUNS = {}


def _runs(name):
    """the float64 and the float32 run of a case, once per session"""
    if name not in _RUNS:
        C, cfg, inp, scales = D.case(name)
        s64, s32 = {}, {}
        g64 = D.reference_grads(C, cfg, inp, scales=scales, stats=s64)
        g32 = D.reference_grads(C, cfg, inp, dtype=torch.float32, scales=scales, stats=s32)
        _RUNS[name] = (inp, g64, g32, s64, s32)
    return _RUNS[name]


@pytest.mark.parametrize("name", list(D.CASES) + list(D.CMD_KINDS) + list(D.POS_KINDS))
def test_populations_margins_and_the_float32_rule(name):
    inp, g64, g32, s64, s32 = _runs(name)
    # the float32 run of the restatement takes the float64 run's branch at every evaluation of every select: no lane is nearer to a
    # boundary than the margin at which fp32 arithmetic of this kind decides alike
    assert D.same_branches(s64, s32) == [], name
    for key in D.KIND_SELECTS.get(name, ()):
        far, near = D.far_lanes(s64, key)
        print(name, key, "far", int(far.sum()), "near", int(near.sum()), "margin", s64["margin"][key])
        assert far.sum() >= 8 and near.sum() >= 8, (name, key)
        assert not far[~inp.rare].any() or key.startswith("rotor"), "only the rare lanes cross the select (the rotor clip: any lane may)"
    if inp.mode == "pos":        # Shepperd's cases 1 and 3 cannot be reached through gpd_ctbr_outer (the helper's docstring)
        assert not D.far_lanes(s64, "shepperd_c1")[0].any() and not D.far_lanes(s64, "shepperd_c3")[0].any()
    err = D.group_errors(g32, g64)
    print(name, "float32 restatement against float64:", {k: f"{v:.2e}" for k, v in err.items()})
    assert max(err.values()) <= F32_RULE, (name, err)
    assert all(np.isfinite(g64[k]).all() for k in D.GROUPS)


# ---- 2. the adjoint text on the host -------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def diff_ctbr_host():
    from gym_pybullet_drones_amd import _native
    return host_lib.program("diff_ctbr_host", include=(_native.CSRC,))


def _clean(run):
    assert "ERROR: AddressSanitizer" not in run.stderr and "runtime error" not in run.stderr, run.stderr[-3000:]


def test_host_side_of_the_entries_under_the_sanitizers(diff_ctbr_host):
    run = host_lib.run(diff_ctbr_host)
    _clean(run)
    print(run.stdout[-1500:])
    assert run.returncode == 0 and "0 checks failed" in run.stdout, run.stdout[-3000:] + run.stderr[-2000:]


def _run_math(exe, what, tmp_path, head: bytes, rows: np.ndarray, width: int) -> np.ndarray:
    src, dst = os.path.join(str(tmp_path), what + ".in"), os.path.join(str(tmp_path), what + ".out")
    with open(src, "wb") as f:
        f.write(struct.pack("<i", len(rows)) + head + np.ascontiguousarray(rows, dtype=np.float32).tobytes())
    run = host_lib.run(exe, what, src, dst)
    _clean(run)
    print(run.stdout.strip())
    assert run.returncode == 0, run.stdout + run.stderr
    return np.fromfile(dst, dtype=np.float32).reshape(len(rows), width).astype(np.float64)


def _figures(got, want, groups):
    return {k: float(np.abs(got[:, s] - want[:, s]).max() / np.abs(want[:, s]).max()) for k, s in groups}


N_MATH = 4096
KF_PLANT = 1.1      # the physics' KF over the controller's nominal one: the rotor chain's derivative is not 1


def _rate_inputs(C, ctl, kind, seed):
    """N_MATH rows (command 4 | body rates 3 | cotangents 4 | plain), every third of `kind`, none within 1e-3 (relative) of a select"""
    rng = np.random.default_rng(seed)
    n = 4 * N_MATH
    cmd = np.hstack([rng.uniform(6.0, 14.0, (n, 1)), rng.uniform(-2.0, 2.0, (n, 3))])
    w = rng.normal(0.0, 1.5, (n, 3))
    # a rate error of 1 rad/s moves a rotor by this fraction of f_max (the racer's yaw axis: 0.73): scaled down to 0.05 per rad/s, or the
    # ordinary rows would sit at the rotor clip too
    per_rad = (ctl.alloc[:, 1:].abs().max(dim=0).values * ctl.J * torch.as_tensor(D.GAINS[3])).numpy() / ctl.f_max
    shrink = np.minimum(1.0, 0.05 / per_rad)
    cmd[:, 1:] *= shrink
    w *= shrink
    rare = np.arange(n) % 3 == 0
    m = int(rare.sum())
    if kind == "thrust_low":
        cmd[rare, 0] = rng.uniform(-6.0, -0.1, m)
    elif kind == "thrust_high":
        cmd[rare, 0] = rng.uniform(41.0, 60.0, m)
    elif kind == "rate_beyond":
        cmd[rare, 1:] = rng.uniform(6.4, 12.0, (m, 3)) * rng.choice([-1.0, 1.0], (m, 3))
    elif kind == "rotor_zero":
        cmd[rare, 0] = rng.uniform(1.0, 5.0, m)
        w[rare] = rng.normal(0.0, 6.0, (m, 3))
    elif kind == "rotor_max":
        cmd[rare, 0] = rng.uniform(17.0, 21.5, m)
        w[rare] = rng.normal(0.0, 6.0, (m, 3))
    else:
        assert kind == "plain"
    cmd, w = (np.asarray(a, dtype=np.float32).astype(np.float64) for a in (cmd, w))
    stats = {}
    T = lambda v: torch.as_tensor(v, dtype=torch.float64)     # noqa: E731
    D.rotor_thrusts(ctl, T(D.GAINS), T(cmd), T(w), stats)
    f = torch.cat([(ctl.M * torch.clamp(T(cmd[:, 0]), 0.0, ctl.thrust_max))[:, None],
                   ctl.J * (T(D.GAINS[3]) * (torch.clamp(T(cmd[:, 1:]), -ctl.rate_max, ctl.rate_max) - T(w))) + torch.cross(T(w), ctl.J * T(w), dim=-1)],
                  dim=-1) @ ctl.alloc.t()
    fr = (f / ctl.f_max).numpy()
    dist = np.minimum.reduce([np.abs(cmd[:, 0]), np.abs(cmd[:, 0] - ctl.thrust_max), np.abs(np.abs(cmd[:, 1:]) - ctl.rate_max).min(axis=1),
                              np.abs(fr).min(axis=1) * 10, np.abs(fr - 1.0).min(axis=1) * 10])
    keep = np.flatnonzero(dist > 1e-2)[:N_MATH]
    assert len(keep) == N_MATH
    inside = (cmd[:, 0] > 0.5) & (cmd[:, 0] < ctl.thrust_max - 0.5) & (np.abs(cmd[:, 1:]) < ctl.rate_max - 0.2).all(axis=1)
    plain = inside & (fr > 0.1).all(axis=1) & (fr < 0.9).all(axis=1)
    ag = np.asarray(rng.standard_normal((n, 4)), dtype=np.float32).astype(np.float64)
    far = {k: np.asarray(v[0]).reshape(n, -1).any(axis=1)[keep] for k, v in stats["masks"].items()}
    return np.hstack([cmd, w, ag, plain[:, None].astype(np.float64)])[keep], far


@pytest.mark.parametrize("kind", ("plain",) + D.CMD_KINDS)
@pytest.mark.parametrize("model", MODELS)
def test_rate_loop_adjoint_in_fp32_against_float64_autograd(diff_ctbr_host, tmp_path, model, kind):
    from gym_pybullet_drones_amd.control.CTBRControl import to_struct
    from gym_pybullet_drones_amd.params import DroneParams
    P, C = DroneParams(_model(model)), H.UrdfConstants(H.URDF[model], model)
    ctl = D.controller(C)
    rows, far = _rate_inputs(C, ctl, kind, seed=11)
    for key in D.KIND_SELECTS.get(kind, ()):
        assert far[key].sum() >= 8 and (~far[key]).sum() >= 8, (kind, key)
    head = bytes(to_struct(P)) + np.array([P.M, P.J[0, 0], P.J[1, 1], P.J[2, 2], KF_PLANT * P.KF], dtype=np.float32).tobytes()
    got = _run_math(diff_ctbr_host, "rate", tmp_path, head, rows, 10)
    leaf = lambda v: torch.tensor(v, dtype=torch.float64, requires_grad=True)     # noqa: E731
    cmd, w, k_rate = leaf(rows[:, 0:4]), leaf(rows[:, 4:7]), leaf(np.tile(D.GAINS[3], (len(rows), 1)))
    gains = [torch.as_tensor(D.GAINS[i], dtype=torch.float64) for i in range(3)] + [k_rate]
    g = (KF_PLANT * C.KF) * ctl.inv_kf * D.rotor_thrusts(ctl, gains, cmd, w)
    want = torch.cat(torch.autograd.grad((torch.as_tensor(rows[:, 7:11]) * g).sum(), (cmd, w, k_rate)), dim=1).numpy()
    err = _figures(got, want, (("command", slice(0, 4)), ("rates", slice(4, 7)), ("k_rate", slice(7, 10))))
    print(model, kind, "MEASURED rate-loop adjoint", {k: f"{v:.2e}" for k, v in err.items()})
    assert np.isfinite(got).all() and max(err.values()) <= TOL, err
    if kind == "thrust_low":      # beyond a clip: exactly zero in the clipped component
        assert (got[far["thrust_lo"], 0] == 0.0).all()
    if kind == "thrust_high":
        assert (got[far["thrust_hi"], 0] == 0.0).all()


def _outer_inputs(C, ctl, kind, seed):
    """N_MATH rows (pos 3 | quat 4 | vel 3 | target pos 3 | target vel 3 | the command's cotangent 4 | plain), every third of `kind`"""
    rng = np.random.default_rng(seed)
    n = 4 * N_MATH
    pos = np.array([0.0, 0.0, 1.0]) + rng.uniform(-0.3, 0.3, (n, 3))
    quat = D.ref.quat_from_rpy(np.hstack([rng.uniform(-0.5, 0.5, (n, 2)), rng.uniform(-3.1, 3.1, (n, 1))])) * rng.uniform(0.97, 1.03, (n, 1))
    vel = rng.uniform(-0.5, 0.5, (n, 3))
    tpos, tvel = pos + rng.uniform(-0.5, 0.5, (n, 3)), rng.uniform(-0.5, 0.5, (n, 3))
    rare = np.arange(n) % 3 == 0
    m = int(rare.sum())
    if kind == "shepperd_c2":
        tpos[rare, 2] = pos[rare, 2] - rng.uniform(1.8, 4.0, m)
        flip = np.tile(np.array([0.0, 1.0, 0.0, 0.0]), (m, 1))
        quat[rare] = D._qmul(flip, D.ref.quat_from_rpy(rng.uniform(-0.5, 0.5, (m, 3))))
    elif kind == "qe_neg":
        quat[rare] = -quat[rare]
    else:
        assert kind == "plain"
    x = np.asarray(np.hstack([pos, quat, vel, tpos, tvel]), dtype=np.float32).astype(np.float64)
    stats = {}
    T = lambda v: torch.as_tensor(v, dtype=torch.float64)     # noqa: E731
    D.outer(ctl, T(D.GAINS), T(x[:, 0:3]), T(x[:, 3:7]), T(x[:, 7:10]), T(x[:, 10:13]), T(x[:, 13:16]), stats)
    # distances to the selects, recomputed here per row: the trace and q_e.w (stats keeps only their minima)
    far = {k: np.asarray(v[0]) for k, v in stats["masks"].items()}
    tr, ew = _trace_and_ew(ctl, x)
    keep = np.flatnonzero((np.abs(tr) > 0.05) & (np.abs(ew) > 0.05))[:N_MATH]
    assert len(keep) == N_MATH
    plain = ~far["shepperd_c2"] & (tr > 0.5) & (np.abs(ew) > 0.3)
    ac = np.asarray(rng.standard_normal((n, 4)), dtype=np.float32).astype(np.float64)
    return np.hstack([x, ac, plain[:, None].astype(np.float64)])[keep], {k: v[keep] for k, v in far.items()}


def _trace_and_ew(ctl, x):
    acc = D.GAINS[0] * (x[:, 10:13] - x[:, 0:3]) + D.GAINS[1] * (x[:, 13:16] - x[:, 7:10]) + np.array([0.0, 0.0, ctl.g])
    zb = acc / np.linalg.norm(acc, axis=1, keepdims=True)
    xb = np.cross(np.array([0.0, 1.0, 0.0]), zb)
    xb /= np.linalg.norm(xb, axis=1, keepdims=True)
    yb = np.cross(zb, xb)
    yb /= np.linalg.norm(yb, axis=1, keepdims=True)
    Rt = np.stack([xb, yb, zb], axis=-1)
    Re = np.einsum("nji,njk->nik", H._rot(x[:, 3:7]), Rt)
    tr = Rt[:, 0, 0] + Rt[:, 1, 1] + Rt[:, 2, 2]
    cos_half = 0.5 * np.sqrt(np.maximum(1.0 + (Re[:, 0, 0] + Re[:, 1, 1] + Re[:, 2, 2]) / np.sum(x[:, 3:7] ** 2, axis=1), 0.0))
    return tr, cos_half          # (|q_e.w| / |q|: its distance from 0, whichever its sign)


@pytest.mark.parametrize("kind", ("plain",) + D.POS_KINDS)
@pytest.mark.parametrize("model", MODELS)
def test_outer_loop_adjoint_in_fp32_against_float64_autograd(diff_ctbr_host, tmp_path, model, kind):
    from gym_pybullet_drones_amd.control.CTBRControl import to_struct
    from gym_pybullet_drones_amd.params import DroneParams
    P, C = DroneParams(_model(model)), H.UrdfConstants(H.URDF[model], model)
    ctl = D.controller(C)
    rows, far = _outer_inputs(C, ctl, kind, seed=13)
    for key in D.KIND_SELECTS.get(kind, ()):
        assert far[key].sum() >= 8 and (~far[key]).sum() >= 8, (kind, key)
    assert not far["shepperd_c1"].any() and not far["shepperd_c3"].any()
    got = _run_math(diff_ctbr_host, "outer", tmp_path, bytes(to_struct(P)), rows, 25)
    leaf = lambda v: torch.tensor(v, dtype=torch.float64, requires_grad=True)     # noqa: E731
    xs = [leaf(rows[:, a:b]) for a, b in ((0, 3), (3, 7), (7, 10), (10, 13), (13, 16))]
    gains = [leaf(np.tile(D.GAINS[i], (len(rows), 1))) for i in range(3)]
    cmd = D.outer(ctl, gains, *xs)
    want = torch.cat(torch.autograd.grad((torch.as_tensor(rows[:, 16:20]) * cmd).sum(), xs + gains), dim=1).numpy()
    err = _figures(got, want, (("pos", slice(0, 3)), ("quat", slice(3, 7)), ("vel", slice(7, 10)), ("target_pos", slice(10, 13)),
                               ("target_vel", slice(13, 16)), ("k_p", slice(16, 19)), ("k_d", slice(19, 22)), ("k_rates", slice(22, 25))))
    print(model, kind, "MEASURED outer-loop adjoint", {k: f"{v:.2e}" for k, v in err.items()})
    assert np.isfinite(got).all() and max(err.values()) <= TOL, err


# ---- 3. binding and refusals ---------------------------------------------------------------------------------------------------------
ENTRIES = ("gpd_rollout_tape_ctbr_floats", "gpd_rollout_tape_ctbr", "gpd_rollout_vjp_ctbr")


def _entries():
    from gym_pybullet_drones_amd import _native
    from gym_pybullet_drones_amd.params import DroneParams
    return _native, _native.lib(), DroneParams().to_struct()


def _expect(L, rc, code, text):
    msg = L.gpd_last_error().decode()
    assert rc == code and text in msg, (rc, msg)


def _cfg(_native, **kw):
    d = dict(num_envs=100, drones_per_env=1, act_type=5, substeps=5, physics_flags=0, pyb_dt=1 / 240, ctrl_dt=1 / 48, inv_ctrl_dt=48.0, task=0)
    d.update(kw)
    return _native.GpdStepCfg(**d)


def test_entries_are_bound_and_the_new_sources_are_tracked():
    _native, L, _ = _entries()
    assert L.gpd_abi_version() == 9 == _native.ABI_VERSION and len(_native.UNITS) == 5
    for name in ENTRIES:
        assert name in _native.exported_symbols() and getattr(L, name).argtypes is not None
    for inc in ("ctbr_vjp.inc", "diff_ctbr_kernels.inc"):
        assert inc in _native.HEADERS and os.path.exists(os.path.join(_native.CSRC, inc))
    abi = open(os.path.join(_native.CSRC, "abi.hip")).read()
    assert abi.index('"diff_kernels.inc"') < abi.index('"ctbr.inc"') < abi.index('"diff_ctbr_kernels.inc"')
    hdr = open(os.path.join(REPO, "include", "gpd.h")).read()
    assert all(f"int {name}(" in hdr for name in ENTRIES)
    from gym_pybullet_drones_amd import diff, engine
    from gym_pybullet_drones_amd.envs.VectorAviary import VectorAviary
    assert diff.CTBR_GAIN_FIELDS == D.GAIN_FIELDS and callable(engine.SimCore.rollout_diff_ctbr) and callable(VectorAviary.rollout_diff_ctbr)


def test_the_tape_is_13_floats_per_drone_step():
    _native, L, _ = _entries()
    out = ctypes.c_int64(0)
    for K, ld in ((1, 128), (8, 128), (20, 65536), (3, 100)):
        assert L.gpd_rollout_tape_ctbr_floats(ctypes.byref(_cfg(_native)), K, ld, ctypes.byref(out)) == 0 and out.value == 13 * K * ld
    E, U = _native.GPD_EINVAL, _native.GPD_ENOTSUP
    _expect(L, L.gpd_rollout_tape_ctbr_floats(None, 4, 128, ctypes.byref(out)), E, "gpd_rollout_tape_ctbr_floats: NULL")
    _expect(L, L.gpd_rollout_tape_ctbr_floats(ctypes.byref(_cfg(_native)), 4, 128, None), E, "gpd_rollout_tape_ctbr_floats: NULL")
    _expect(L, L.gpd_rollout_tape_ctbr_floats(ctypes.byref(_cfg(_native)), 0, 128, ctypes.byref(out)), E, "num_steps must be positive")
    _expect(L, L.gpd_rollout_tape_ctbr_floats(ctypes.byref(_cfg(_native)), 4, 99, ctypes.byref(out)), E, "ld < num_envs")
    for flag in (1, 2, 4, 8, 16):
        _expect(L, L.gpd_rollout_tape_ctbr_floats(ctypes.byref(_cfg(_native, physics_flags=flag)), 4, 128, ctypes.byref(out)), U, "physics_flags")
    _expect(L, L.gpd_rollout_tape_ctbr_floats(ctypes.byref(_cfg(_native, physics_flags=32)), 4, 128, ctypes.byref(out)), E, "unknown physics flag")


def test_gpd_rollout_tape_ctbr_rejects_bad_arguments_without_a_device():
    _native, L, params = _entries()
    b = _native.GpdCtbr()
    p, odd = ctypes.c_void_p(0x1000), ctypes.c_void_p(0x1004)      # never dereferenced: every call below fails its checks first

    def call(state_kw=None, cfg_kw=None, ctbr=ctypes.byref(b), mode=0, rows=p, rs=0, plant=None, obs=p, os_=0, cmd=None, K=4, tape=ctypes.c_void_p(0x100000)):
        st = _native.GpdState(kin=0x1000, last_rpm=0x1000, step_counter=0x1000, ld=128)
        for k, v in (state_kw or {}).items():
            setattr(st, k, v)
        return L.gpd_rollout_tape_ctbr(ctypes.byref(params), ctbr, ctypes.byref(st), ctypes.byref(_cfg(_native, **(cfg_kw or {}))), mode, rows, rs, plant,
                                       obs, os_, cmd, K, tape, None)
    E, R, U = _native.GPD_EINVAL, _native.GPD_ERANGE, _native.GPD_ENOTSUP
    _expect(L, L.gpd_rollout_tape_ctbr(None, None, None, None, 0, None, 0, None, None, 0, None, 0, None, None), E, "gpd_rollout_tape_ctbr: NULL")
    _expect(L, call(ctbr=None), E, "gpd_rollout_tape_ctbr: NULL params/ctbr/state/cfg")
    _expect(L, call(state_kw=dict(kin=None)), E, "gpd_rollout_tape_ctbr: NULL state.kin")
    for kw in (dict(rows=None), dict(obs=None), dict(tape=None)):
        _expect(L, call(**kw), E, "gpd_rollout_tape_ctbr: NULL rows/obs12/tape")
    _expect(L, call(state_kw=dict(kin=0x1004)), E, "16-byte aligned")
    _expect(L, call(mode=2), E, "gpd_rollout_tape_ctbr: unknown mode")
    _expect(L, call(K=0), E, "num_steps must be positive")
    _expect(L, call(rs=-4), E, "non-negative")
    _expect(L, call(cfg_kw=dict(num_envs=0)), E, "must be positive")
    _expect(L, call(cfg_kw=dict(substeps=0)), E, "must be positive")
    _expect(L, call(cfg_kw=dict(physics_flags=32)), E, "unknown physics flag")
    # GPD_ENOTSUP where gpd_rollout_ctbr answers it ...
    _expect(L, call(cfg_kw=dict(drones_per_env=2, num_envs=50)), U, "drones_per_env")
    _expect(L, call(cfg_kw=dict(task=1)), U, "GPD_TASK_NONE")
    _expect(L, call(cfg_kw=dict(auto_reset=1)), U, "auto_reset")
    for act in (0, 1, 2, 3, 4):
        _expect(L, call(cfg_kw=dict(act_type=act)), U, "act_type")
    _expect(L, call(state_kw=dict(dw_force=0x1000)), U, "dw_force")
    # ... and for every physics flag
    for flag in (1, 2, 4, 8, 16, 3, 31):
        _expect(L, call(cfg_kw=dict(physics_flags=flag)), U, "gpd_rollout_tape_ctbr: physics_flags are not differentiable")
    _expect(L, call(state_kw=dict(ld=99)), E, "ld")
    _expect(L, call(cfg_kw=dict(num_envs=(1 << 26) + 1), state_kw=dict(ld=1 << 27)), R, "2^26")
    _expect(L, call(rs=396), E, "step stride")                 # CMD: 4 * 100 floats per step
    _expect(L, call(mode=1, rs=400), E, "step stride")         # POS: 12 * 100
    _expect(L, call(os_=400), E, "step stride")
    _expect(L, call(rs=402), E, "multiples of 4")
    _expect(L, call(os_=1201), E, "multiples of 4")
    for kw in (dict(rows=odd), dict(obs=odd), dict(plant=odd), dict(cmd=odd), dict(tape=odd)):
        _expect(L, call(**kw), E, "16-byte aligned")
    _expect(L, call(cmd=p), E, "must not alias")
    _expect(L, call(cfg_kw=dict(ctrl_dt=0.0)), E, "must be positive")
    _expect(L, call(cfg_kw=dict(pyb_dt=0.0)), E, "must be positive")


def test_gpd_rollout_vjp_ctbr_rejects_bad_arguments_without_a_device():
    _native, L, params = _entries()
    b = _native.GpdCtbr()
    V = ctypes.c_void_p
    odd = V(0x1004)
    ok = dict(rows=V(0x1000), tape=V(0x1000000), g_obs=V(0x2000000), g_kin=V(0x3000000), g_rows=V(0x4000000), g_gains=None, plant=None)

    def call(cfg_kw=None, ctbr=ctypes.byref(b), ld=128, mode=0, K=4, rs=0, os_=1200, **ptr):
        a = {**ok, **ptr}
        return L.gpd_rollout_vjp_ctbr(ctypes.byref(params), ctbr, ctypes.byref(_cfg(_native, **(cfg_kw or {}))), ld, mode, K, a["rows"], rs, a["plant"],
                                      a["tape"], a["g_obs"], os_, a["g_kin"], a["g_rows"], a["g_gains"], None)
    E, R, U = _native.GPD_EINVAL, _native.GPD_ERANGE, _native.GPD_ENOTSUP
    _expect(L, L.gpd_rollout_vjp_ctbr(None, None, None, 0, 0, 0, None, 0, None, None, None, 0, None, None, None, None), E, "gpd_rollout_vjp_ctbr: NULL")
    _expect(L, call(ctbr=None), E, "gpd_rollout_vjp_ctbr: NULL params/ctbr/cfg")
    for kw in (dict(rows=None), dict(tape=None), dict(g_kin=None), dict(g_rows=None)):
        _expect(L, call(**kw), E, "gpd_rollout_vjp_ctbr: NULL rows/tape/g_kin/g_rows")
    _expect(L, call(mode=-1), E, "gpd_rollout_vjp_ctbr: unknown mode")
    _expect(L, call(K=0), E, "num_steps must be positive")
    _expect(L, call(rs=-4), E, "non-negative")
    _expect(L, call(os_=-12), E, "non-negative")
    _expect(L, call(ld=0), E, "ld must be in")
    _expect(L, call(ld=99), E, "ld < num_envs")
    _expect(L, call(cfg_kw=dict(substeps=0)), E, "must be positive")
    _expect(L, call(cfg_kw=dict(physics_flags=32)), E, "unknown physics flag")
    _expect(L, call(cfg_kw=dict(drones_per_env=2, num_envs=50)), U, "drones_per_env")
    _expect(L, call(cfg_kw=dict(task=1)), U, "GPD_TASK_NONE")
    _expect(L, call(cfg_kw=dict(auto_reset=1)), U, "auto_reset")
    for act in (0, 1, 2, 3, 4):
        _expect(L, call(cfg_kw=dict(act_type=act)), U, "act_type")
    for flag in (1, 2, 4, 8, 16, 3, 31):
        _expect(L, call(cfg_kw=dict(physics_flags=flag)), U, "gpd_rollout_vjp_ctbr: physics_flags are not differentiable")
    _expect(L, call(cfg_kw=dict(num_envs=(1 << 26) + 1), ld=1 << 27), R, "2^26")
    _expect(L, call(rs=396), E, "step stride")
    _expect(L, call(mode=1, rs=400), E, "step stride")
    _expect(L, call(os_=400), E, "step stride")
    _expect(L, call(rs=402), E, "multiples of 4")
    for kw in (dict(rows=odd), dict(plant=odd), dict(tape=odd), dict(g_obs=odd), dict(g_kin=odd), dict(g_rows=odd), dict(g_gains=odd)):
        _expect(L, call(**kw), E, "16-byte aligned")
    # g_kin is 13 ld floats, the tape 13 ld K, g_rows 4 N K (12 N K in POS), g_gains 12 ld: none may share a word with another
    for kw in (dict(g_rows=ok["g_kin"]), dict(g_gains=ok["g_kin"]), dict(g_gains=ok["g_rows"]), dict(g_kin=ok["tape"]), dict(g_rows=ok["tape"]),
               dict(g_gains=ok["tape"]), dict(g_kin=V(0x1000000 + 13 * 128 * 4 * 3)), dict(g_gains=V(0x4000000 + 4 * 100 * 4 * 4 - 16)),
               dict(g_rows=V(0x3000000 + 13 * 128 * 4 - 16))):
        _expect(L, call(**kw), E, "gpd_rollout_vjp_ctbr: g_rows, g_gains, g_kin and tape must not alias")
    assert L.gpd_rollout_vjp_ctbr.argtypes[-1] is ctypes.c_void_p and len(L.gpd_rollout_vjp_ctbr.argtypes) == 16


def test_rollout_diff_ctbr_refuses_before_any_device_work():
    from gym_pybullet_drones_amd import engine
    from gym_pybullet_drones_amd.control import VectorCTBR
    from gym_pybullet_drones_amd.envs.VectorAviary import VectorAviary
    cpu = torch.device("cpu")
    ctrl = VectorCTBR(4, _model("cf2x"), device=cpu)

    def core(**kw):         # what rollout_diff_ctbr reads of a SimCore before its first call into the library
        return types.SimpleNamespace(**{"N": 4, "device": cpu, "host_visible": False, "act_ring": None, **kw})
    roll = engine.SimCore.rollout_diff_ctbr
    cmd = torch.zeros((4, 4))
    cases = ((core(), (ctrl, cmd), dict(num_steps=0)), (core(), (ctrl, cmd), {}), (core(), (ctrl, cmd), dict(num_steps=3, mode="rates")),
             (core(host_visible=True), (ctrl, cmd), dict(num_steps=3)), (core(act_ring=cmd), (ctrl, cmd), dict(num_steps=3)),
             (core(N=5), (ctrl, torch.zeros((5, 4))), dict(num_steps=3)), (core(), (object(), cmd), dict(num_steps=3)),
             (core(), (ctrl, torch.zeros((4, 12))), dict(num_steps=3)), (core(), (ctrl, torch.zeros((2, 4, 4))), dict(num_steps=3)),
             (core(), (ctrl, cmd), dict(num_steps=3, mode="pos")), (core(), (ctrl, torch.zeros((3, 4, 5))), dict(mode="pos")),
             (core(), (ctrl, cmd), dict(num_steps=3, gains=torch.zeros(6, 3))), (core(), (ctrl, cmd), dict(num_steps=3, gains=[1.0] * 12)))
    for who, args, kw in cases:
        with pytest.raises((ValueError, AttributeError)) as e:
            roll(who, *args, **kw)
        assert e.type is ValueError, (args[1:], kw, e.value)
        env = types.SimpleNamespace(core=types.SimpleNamespace(rollout_diff_ctbr=lambda *a, _who=who: roll(_who, *a)), NUM_ENVS=4, NUM_DRONES=1)
        with pytest.raises(ValueError):
            VectorAviary.rollout_diff_ctbr(env, *args, **kw)
