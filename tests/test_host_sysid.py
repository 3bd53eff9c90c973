"""Gradients with respect to the plant scales without a GPU: the float64 yardstick (tests/helpers/diff_f64.py with the scales as
autograd leaves: `consts(scales=)`, `reference_grads(wrt_scales=True)`) against finite differences, its float32 run against its
float64 run on the GPU tests' inputs, the scaling identity, and the host side of the two entries (include/gpd.h
`gpd_rollout_vjp_plant` / `gpd_plant_derive_vjp`): every refusal with its code and message, tests/c/diff_host.c under AddressSanitizer
+ UBSan against the launch stub, the formulas of csrc/plant_derive_vjp.inc against a numerical Jacobian, and the compiler's word that
no kernel of the sweep needs scratch memory."""
import ctypes
import os
import re
import subprocess
import sys
import tempfile

import numpy as np
import pytest
import torch

from conftest import REPO

sys.path.insert(0, os.path.join(REPO, "tests", "helpers"))
import diff_f64 as ref  # noqa: E402
import host_lib  # noqa: E402
from host_lib import REJECTED, params as _params, step_cfg as _cfg  # noqa: E402
import sysid_f64 as sid  # noqa: E402


# ---- the yardstick -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("model,act,drag,S", [("cf2x", "rpm", True, 2), ("racer", "one_d_rpm", False, 1), ("cf2p", "raw_rpm", True, 1)])
def test_restatement_scale_gradients_pass_gradcheck(model, act, drag, S):
    """float64 autograd of the restatement with respect to the [9, n] scales against finite differences: 2 drones, K = 3"""
    C = _params(model)
    cfg = ref.config(model, act, S, drag, "hover")
    inp = ref.make_inputs(C, cfg, 2, 3, seed=5, outside_clip=False)
    T = lambda v: torch.as_tensor(v, dtype=torch.float64)     # noqa: E731
    kin0 = tuple(T(v) for v in (inp.pos, inp.quat, inp.vel, inp.rates))

    def f(s):
        obs, rew, kin = ref.rollout(ref.consts(C, 2, scales=s), cfg, kin0, T(inp.actions), T(inp.first_sum), T(inp.target))
        return torch.cat([obs.reshape(-1), rew.reshape(-1)] + [k.reshape(-1) for k in kin])

    s = T(np.random.default_rng(7).uniform(0.8, 1.2, (9, 2))).requires_grad_(True)
    assert torch.autograd.gradcheck(f, [s], eps=1e-6, atol=1e-6, rtol=1e-5)


@pytest.fixture(scope="module")
def runs():
    """every run of the GPU tests once: the float64 scale gradients and the float32 run of the same restatement"""
    out = {}
    for name, ones in sid.RUNS:
        cfg, K, scales = sid.case(name, ones=ones)
        C = _params(cfg.model)
        inp = ref.make_inputs(C, cfg, 70, K, seed=1)
        g64, g32 = (ref.reference_grads(C, cfg, inp, dtype, scales, wrt_scales=True)["scales"] for dtype in (torch.float64, torch.float32))
        out[name, ones] = (cfg, scales, g64, g32)
    return out


@pytest.mark.parametrize("name,ones", sid.RUNS)
def test_float32_restatement_follows_the_float64_one_on_the_gpu_inputs(runs, name, ones):
    """what float32 costs on these inputs, measured on the restatement itself: max |g32 - g64| / max |g64| per scale stays below 1e-5
    (measured: <= 2.5e-6), so that a device gradient within 1e-4 of the float64 one is a statement about the kernel.  Scales the
    configuration does not read have a gradient of exactly zero in the reference too."""
    cfg, _, g64, g32 = runs[name, ones]
    err = sid.scale_errors(g32, g64)
    print(name, "ones" if ones else "random", {k: f"{v:.1e}" for k, v in err.items()})
    assert max(err.values()) < 1e-5, err
    assert np.isfinite(g64).all()
    read = set(err) | ({"km"} if cfg.act == "one_d_rpm" else set())          # (four equal thrusts: no yaw torque, whatever KM is)
    assert read == set(sid.SCALES) - {"gnd_eff"} - (set() if cfg.drag else {"drag_xy", "drag_z"}), read


@pytest.mark.parametrize("name,ones", sid.RUNS)
def test_scaling_identity_holds_in_float64(runs, name, ones):
    """mass, the inertias, KF, KM and the drag coefficients scaled by one factor change nothing (every force, every torque and every
    inertia scale alike; the RPMs do not depend on the plant): sum_{i<8} s_i g_i = 0 per drone.  Measured 3.5e-15 of sum |s_i g_i|;
    the bound leaves float64 three decades for a few hundred operations."""
    _, scales, g64, _ = runs[name, ones]
    terms = scales[:8] * g64[:8]
    rel = np.abs(terms.sum(axis=0)) / np.abs(terms).sum(axis=0)
    print(name, "ones" if ones else "random", f"{rel.max():.1e}")
    assert rel.max() < 1e-12


# ---- the host side of the entries -------------------------------------------------------------------------------------------------
def test_new_entries_are_bound_and_the_abi_version_stays():
    from gym_pybullet_drones_amd import _native
    assert _native.ABI_VERSION == 9 and _native.lib().gpd_abi_version() == 9
    assert {"gpd_rollout_vjp_plant", "gpd_plant_derive_vjp"} <= set(_native.exported_symbols())
    assert "plant_derive_vjp.inc" in _native.HEADERS


def test_every_refusal_returns_its_code_and_an_entry_named_message():
    """gpd_rollout_vjp_plant: gpd_rollout_vjp's refusals (GPD_ENOTSUP for what diff_cfg refuses, GPD_EINVAL for bad arguments) and its
    own (no plant table, no / a misaligned g_plant_rows); gpd_plant_derive_vjp: NULL pointers, n, ld.  The pointers are fake addresses
    of host memory: a call that got as far as a launch would not return a negative code on a machine without a device
    (tests/c/diff_host.c counts the launches against the stub: none)."""
    from gym_pybullet_drones_amd import _native
    from gym_pybullet_drones_amd.utils.enums import DroneModel
    L = _native.lib()
    P = _params("cf2x").to_struct(pid_model=DroneModel.CF2X)
    buf = (ctypes.c_float * 64)()
    p = ctypes.cast(buf, ctypes.c_void_p)
    odd = ctypes.c_void_p(p.value + 4)

    def vjp(cfg=None, K=4, ld=128, plant=p, g_plant=p, g_kin=p, g_act=p, tape=p, target=p, a_stride=280):
        cfg = _cfg() if cfg is None else cfg
        rc = L.gpd_rollout_vjp_plant(ctypes.byref(P), ctypes.byref(cfg), ld, K, p, a_stride, target, plant, tape, p, 840, p, 70, g_kin, g_act, g_plant, None)
        return rc, L.gpd_last_error().decode()

    for change, reason in REJECTED:
        rc, msg = vjp(_cfg(**change))
        assert rc == _native.GPD_ENOTSUP and msg.startswith("gpd_rollout_vjp_plant:") and reason in msg, (change, rc, msg)
    for kw, reason in ((dict(plant=None), "plant_rows"), (dict(g_plant=None), "g_plant_rows"), (dict(g_plant=odd), "g_plant_rows must be 16-byte"),
                       (dict(plant=odd), "plant_rows must be 16-byte"), (dict(K=0), "num_steps"), (dict(ld=64), "ld"), (dict(g_kin=None), "NULL"),
                       (dict(g_kin=odd), "16-byte"), (dict(g_act=None), "NULL"), (dict(g_act=odd), "16-byte"), (dict(tape=None), "NULL"),
                       (dict(tape=odd), "16-byte"), (dict(target=None), "target_pos"), (dict(a_stride=-1), "strides")):
        rc, msg = vjp(**kw)
        assert rc == _native.GPD_EINVAL and msg.startswith("gpd_rollout_vjp_plant:") and reason in msg, (kw, rc, msg)
    rc, msg = vjp(_cfg(num_envs=(1 << 26) + 1), ld=(1 << 26) + 64)
    assert rc == _native.GPD_ERANGE and msg.startswith("gpd_rollout_vjp_plant:") and "2^26" in msg

    def derive(nominal=ctypes.byref(P), scales=p, g_rows=p, n=70, ld=128, g_scales=p):
        rc = L.gpd_plant_derive_vjp(nominal, scales, g_rows, n, ld, g_scales, None)
        return rc, L.gpd_last_error().decode()

    for kw, reason in ((dict(nominal=None), "NULL"), (dict(scales=None), "NULL"), (dict(g_rows=None), "NULL"), (dict(g_scales=None), "NULL"),
                       (dict(n=0), "n must"), (dict(n=-5), "n must"), (dict(ld=64), "ld"), (dict(ld=0), "ld"), (dict(ld=1 << 32), "ld")):
        rc, msg = derive(**kw)
        assert rc == _native.GPD_EINVAL and msg.startswith("gpd_plant_derive_vjp:") and reason in msg, (kw, rc, msg)
    rc, msg = derive(n=(1 << 26) + 1, ld=(1 << 26) + 64)
    assert rc == _native.GPD_ERANGE and msg.startswith("gpd_plant_derive_vjp:") and "2^26" in msg


@pytest.fixture(scope="module")
def host_program():
    """tests/c/diff_host.c linked to the host-only build of the five units and the launch stub under -fsanitize=address,undefined and
    run once (tests/helpers/host_lib.py; shared with tests/test_host_diff.py): (the finished process, the file of formula values)"""
    return host_lib.diff_host()


def test_host_side_of_the_plant_gradient_entries_under_asan_and_ubsan(host_program):
    """accepted and rejected arguments, and the kernel each accepted call launches: the four GP instantiations and the derive-vjp kernel"""
    run, _ = host_program
    print(run.stdout[-6000:])
    assert "AddressSanitizer" not in run.stderr and "runtime error" not in run.stderr, run.stderr[-4000:]
    assert run.returncode == 0 and "\n0 checks failed" in run.stdout, run.stdout[-3000:] + run.stderr[-2000:]
    assert run.stdout.count("\nok ") + run.stdout.startswith("ok ") >= 50 + 60          # (this module's entries + the three they extend)
    for inst in ("<EXT 0, AW 4, PLANT 1, GP 1>", "<EXT 0, AW 1, PLANT 1, GP 1>", "<EXT 1, AW 1, PLANT 1, GP 1>", "<EXT 1, AW 4, PLANT 1, GP 1>"):
        assert any(line.startswith("ok ") and inst in line for line in run.stdout.split("\n")), inst
    assert "ok   gpd_plant_derive_vjp launches its kernel once" in run.stdout


def test_derive_vjp_formulas_are_the_transpose_jacobian_of_the_derive_formulas(host_program):
    """csrc/plant_derive_vjp.inc -- the text gpd_plant_derive_vjp_kernel compiles -- evaluated by the stand-alone program on 64 drones
    (scales in [0.5, 2), cotangents in [-1, 1)), against J(s)^T g with J the complex-step Jacobian of the numpy float64 statement of
    gpd_plant_derive: 1e-13 of the largest term (float64, a dozen operations per output)"""
    run, values = host_program
    assert run.returncode == 0, run.stdout[-2000:]
    lines = open(values).read().strip().split("\n")
    n = [float(np.float32(x)) for x in lines[0].split()]          # (nine digits name a float32; the formulas read the float32)
    nom = dict(M=n[0], inv_M=n[1], KF=n[2], GRAVITY=n[3], J=n[4:7], J_INV=n[7:10], km_over_kf=n[10], gnd_eff_coeff=n[11], drag_coeff=n[12:15],
               hover_thrust=n[15], hover_resid=n[16])
    table = np.array([[float(x) for x in line.split()] for line in lines[1:]])
    assert table.shape == (64, 9 + 19 + 9)
    s, g, got = table[:, :9].T, table[:, 9:28].T, table[:, 28:].T
    want = sid.derive_vjp_numeric(nom, s, g)
    # (the derive formulas themselves: scales of one give the nominal fields, NORM_GAP exactly +0)
    one = sid.derive(nom, np.ones((9, 1)))[:, 0]
    assert one[0] == nom["M"] and one[10] == nom["km_over_kf"] and one[16] == nom["hover_resid"] and one[18] == 0.0 and one[17] == nom["hover_thrust"]
    scale = np.zeros_like(want)
    for k in range(9):
        z = s.astype(np.complex128)
        z[k] += 1e-30j
        scale[k] = np.abs(sid.derive(nom, z).imag / 1e-30 * g).sum(axis=0)
    err = np.abs(got - want) / scale
    print("max error relative to the sum of |terms| per scale:", err.max(axis=1))
    assert err.max() < 1e-13 and np.abs(want).min() > 0


def test_no_kernel_of_the_reverse_sweep_needs_scratch_memory():
    """`-Rpass-analysis=kernel-resource-usage` on abi.hip: the eight gpd_rollout_vjp_kernel instantiations that were there, the four with
    the plant rows' cotangents (16 more accumulators per lane) and gpd_plant_derive_vjp_kernel all report ScratchSize 0"""
    from gym_pybullet_drones_amd import _native
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    if not os.path.exists(hipcc):
        pytest.skip("no hipcc")
    unit, extra = next(u for u in _native.UNITS if u[0] == "abi.hip")
    flags = [f for f in _native.COMMON_FLAGS if f != "-fPIC"] + extra
    with tempfile.TemporaryDirectory() as d:
        res = subprocess.run([hipcc] + flags + ["-S", "--cuda-device-only", "-Rpass-analysis=kernel-resource-usage", "-I",
                                                os.path.join(REPO, "include"), os.path.join(_native.CSRC, unit), "-o", os.path.join(d, "u.s")],
                             check=True, capture_output=True, text=True)
    found = {}
    name = None
    for line in res.stderr.split("\n"):
        m = re.search(r"Function Name: (\S+)", line)
        if m:
            name = m.group(1)
        m = re.search(r"ScratchSize \[bytes/lane\]: (\d+)", line)
        if m and name and ("gpd_rollout_vjp_kernel" in name or "gpd_plant_derive_vjp_kernel" in name):
            found[name] = int(m.group(1))
    sweep = sorted(k for k in found if "gpd_rollout_vjp_kernel" in k)
    assert len(sweep) == 12 and len(found) == 13, sorted(found)
    assert sum("ELb1ELb1EEEv" in k for k in sweep) == 4 and sum("ELb0EEEv" in k for k in sweep) == 8, sweep      # <.., PLANT 1, GP 1>; <.., GP 0>
    assert all(v == 0 for v in found.values()), found
