"""ctypes binding of `csrc/libgpd.so` (the C-ABI declared in include/gpd.h).

There is NO fallback: if the library is missing or does not match the header, importing the
product path raises.  `build()` compiles it in-tree with hipcc for gfx950 (cross-compiles on a
machine without a GPU).
"""
import contextlib
import ctypes
import os
import subprocess

try:        # PyTorch's HIP runtime first: libgpd.so then binds to the copy torch mapped (one runtime per process; loaded the other way
    import torch  # round, a kernel launch fails with "no ROCm-capable device is detected": round 5)
except ImportError:     # (setup.py compiles the library through build() where torch need not be installed)
    torch = None

from .params import GpdParams

_HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(_HERE, "csrc")
INCLUDE = os.path.join(os.path.dirname(_HERE), "include")        # the source tree's include/ ...
if not os.path.exists(os.path.join(INCLUDE, "gpd.h")):            # ... or the copy setup.py puts inside an installed package
    INCLUDE = os.path.join(_HERE, "include")
LIB_PATH = os.path.join(CSRC, "libgpd.so")
ABI_VERSION = 9

# Five translation units over csrc/gpd_common.inc (the shared physics), one library:
#   step_rollout.hip  gpd_step / gpd_rollout*            -mllvm -amdgpu-sched-strategy=max-ilp: interleaves independent dependency chains, which
#                     fills the one-wait-state hazard behind every packed-fp32 result with useful work instead of s_nops (13 of 287 issue
#                     slots of a rollout step)
#   policy.hip        gpd_rollout_policy                 the default scheduler: 10 % faster on its MFMA + activation mix (round-2 A/B)
#   swarm.hip         the one-world kernels              max-ilp, as in rounds 2-4
#   abi.hip           small kernels, RCCL, library-level entries; the differentiable rollout (RPM and DSLPID), gpd_obstacles, gpd_rollout_obst, gpd_mppi and the
#                     thrust-and-body-rate controller gpd_ctbr / gpd_rollout_ctbr (as a task: gpd_task_eval / gpd_rollout_ctbr_task) with its planner gpd_mppi_ctbr, gpd_mppi_peers, gpd_mppi_plant and its differentiable
#                     rollout (csrc/*.inc pulled in at its end)
#   mrac.hip          gpd_mrac / gpd_mrac_reset / gpd_rollout_mrac: the adaptive controller and the rollout that carries it (max-ilp)
#   -mllvm -amdgpu-kernarg-preload-count=14: the first 14 argument dwords of a kernel arrive in SGPRs with the wave (gfx942+ command
#   processor) instead of through a scalar load -- gpd_step_kernel's argument list starts with what its load section needs
COMMON_FLAGS = ["-O3", "-std=c++17", "--offload-arch=gfx950", "-ffp-contract=off", "-fno-slp-vectorize", "-fPIC"]
MAX_ILP = ["-mllvm", "-amdgpu-sched-strategy=max-ilp"]
KERNARG_PRELOAD = ["-mllvm", "-amdgpu-kernarg-preload-count=14"]
HIPCC_FLAGS = COMMON_FLAGS + MAX_ILP + ["-shared"]        # (kept under this name for the ISA tests)
UNITS = (("step_rollout.hip", MAX_ILP + KERNARG_PRELOAD), ("policy.hip", []), ("swarm.hip", MAX_ILP + KERNARG_PRELOAD), ("abi.hip", MAX_ILP), ("mrac.hip", MAX_ILP))
HEADERS = ("gpd_common.inc", "policy_kernel.inc", "diff_kernels.inc", "plant_derive_vjp.inc", "diff_pid_kernels.inc", "dslpid_vjp.inc", "obstacle_math.inc", "obstacles.inc", "obst_task_math.inc", "obst_task.inc", "mppi_math.inc", "mppi.inc", "ctbr_math.inc", "ctbr.inc", "ctbr_task.inc", "mppi_ctbr.inc", "mppi_peers_math.inc", "mppi_peers.inc", "mppi_plant.inc", "ctbr_vjp.inc", "diff_ctbr_kernels.inc")


class GpdError(RuntimeError):
    pass


class GpdState(ctypes.Structure):
    """mirror of `struct GpdState`"""
    _fields_ = [("kin", ctypes.c_void_p), ("last_rpm", ctypes.c_void_p), ("pid", ctypes.c_void_p),
                ("step_counter", ctypes.c_void_p), ("ld", ctypes.c_int64), ("dw_force", ctypes.c_void_p),
                ("act_ring", ctypes.c_void_p), ("ring_pos", ctypes.c_void_p), ("hist_len", ctypes.c_int32),
                ("pad_", ctypes.c_int32), ("bad", ctypes.c_void_p)]


class GpdStepCfg(ctypes.Structure):
    """mirror of `struct GpdStepCfg`"""
    _fields_ = [("num_envs", ctypes.c_int32), ("drones_per_env", ctypes.c_int32), ("act_type", ctypes.c_int32),
                ("substeps", ctypes.c_int32), ("physics_flags", ctypes.c_uint32), ("pyb_dt", ctypes.c_float),
                ("ctrl_dt", ctypes.c_float), ("inv_ctrl_dt", ctypes.c_float), ("lanes_per_wave", ctypes.c_int32),
                ("task", ctypes.c_int32), ("xy_bound", ctypes.c_float),
                ("z_bound", ctypes.c_float), ("tilt_bound", ctypes.c_float), ("term_dist", ctypes.c_float),
                ("trunc_counter", ctypes.c_int32), ("target_per_env", ctypes.c_int32),
                ("init_per_env", ctypes.c_int32), ("auto_reset", ctypes.c_int32)]


class GpdP2P(ctypes.Structure):
    """mirror of `struct GpdP2P` (one block of gpd_p2p_group)"""
    _fields_ = [("peer", ctypes.c_int32), ("pad_", ctypes.c_int32), ("ptr", ctypes.c_void_p), ("count", ctypes.c_int64)]


class GpdSwarm(ctypes.Structure):
    """mirror of `struct GpdSwarm`"""
    _fields_ = [("n_rows", ctypes.c_int32), ("slab", ctypes.c_int32), ("world_size", ctypes.c_int32), ("rank", ctypes.c_int32),
                ("own_count", ctypes.c_int32), ("nx", ctypes.c_int32), ("ny", ctypes.c_int32), ("nz", ctypes.c_int32),
                ("cell", ctypes.c_float), ("x0", ctypes.c_float), ("y0", ctypes.c_float), ("z0", ctypes.c_float),
                ("zbin", ctypes.c_float), ("meta_rows", ctypes.c_int32),
                ("pos4", ctypes.c_void_p), ("bin_pos", ctypes.c_void_p), ("cell_count", ctypes.c_void_p),
                ("cell_start", ctypes.c_void_p), ("order", ctypes.c_void_p), ("visit", ctypes.c_void_p), ("visit_out", ctypes.c_void_p),
                ("slot_key", ctypes.c_void_p), ("dw_force", ctypes.c_void_p), ("slot_of", ctypes.c_void_p),
                ("pos_sorted", ctypes.c_void_p), ("pair_list", ctypes.c_void_p), ("pair_nb", ctypes.c_void_p),
                ("list_ok", ctypes.c_void_p), ("list_cap", ctypes.c_int32), ("list_delta", ctypes.c_float),
                ("drift", ctypes.c_void_p), ("total_drones", ctypes.c_int32), ("list_adapt", ctypes.c_int32)]


class GpdMrac(ctypes.Structure):
    """mirror of `struct GpdMrac` (the MRAC design as fp32 constants, control/MRAC.py)"""
    _fields_ = [("PB", ctypes.c_float * 48), ("Kr_ref_gain", ctypes.c_float * 48), ("Am_lo", ctypes.c_float * 48),
                ("A_grav", ctypes.c_float * 4), ("B_diag", ctypes.c_float * 4), ("mixer", ctypes.c_float * 12),
                ("gamma_x", ctypes.c_float), ("gamma_r", ctypes.c_float), ("inv_4kf", ctypes.c_float), ("max_torque", ctypes.c_float),
                ("pwm2rpm_scale", ctypes.c_float), ("inv_pwm2rpm_scale", ctypes.c_float), ("pwm2rpm_const", ctypes.c_float),
                ("min_pwm", ctypes.c_float), ("max_pwm", ctypes.c_float), ("pad_", ctypes.c_float * 3),
                ("Kx0", ctypes.c_float * 48), ("Kr0", ctypes.c_float * 16)]


class GpdMppi(ctypes.Structure):
    """mirror of `struct GpdMppi` (gpd_mppi / gpd_mppi_ctbr: the sampler, the cost's weights, the Philox key and the plan's counter word)"""
    _fields_ = [("horizon", ctypes.c_int32), ("samples", ctypes.c_int32), ("sigma", ctypes.c_float * 4), ("act_lo", ctypes.c_float * 4),
                ("act_hi", ctypes.c_float * 4), ("lam", ctypes.c_float), ("w_pos", ctypes.c_float), ("w_vel", ctypes.c_float),
                ("w_tilt", ctypes.c_float), ("w_rate", ctypes.c_float), ("w_term", ctypes.c_float), ("w_obs", ctypes.c_float),
                ("obst_margin", ctypes.c_float), ("collision_radius", ctypes.c_float), ("seed", ctypes.c_uint32 * 2),
                ("iteration", ctypes.c_uint32)]


class GpdMppiPeers(ctypes.Structure):
    """mirror of `struct GpdMppiPeers` (gpd_mppi_peers: the peers' lists and published paths, the path this call publishes, the hinge)"""
    _fields_ = [("idx", ctypes.c_void_p), ("pos", ctypes.c_void_p), ("path_out", ctypes.c_void_p), ("pos_step_stride", ctypes.c_int64),
                ("k", ctypes.c_int32), ("idx_ld", ctypes.c_int32), ("n_rows", ctypes.c_int32), ("w_peer", ctypes.c_float),
                ("peer_dist", ctypes.c_float)]


class GpdCtbr(ctypes.Structure):
    """mirror of `struct GpdCtbr` (gpd_ctbr / gpd_rollout_ctbr: the outer loop's gains, the rate loop's gains, clips and allocation)"""
    _fields_ = [("k_p", ctypes.c_float * 3), ("k_d", ctypes.c_float * 3), ("k_rates", ctypes.c_float * 3), ("g", ctypes.c_float),
                ("k_rate", ctypes.c_float * 3), ("thrust_max", ctypes.c_float), ("rate_max", ctypes.c_float), ("alloc", ctypes.c_float * 12),
                ("f_max", ctypes.c_float), ("inv_kf", ctypes.c_float), ("pad_", ctypes.c_float * 3)]


class GpdObstTask(ctypes.Structure):
    """mirror of `struct GpdObstTask` (gpd_rollout_obst: contact, the proximity hinge and the range sensor of the obstacle task)"""
    _fields_ = [("collision_radius", ctypes.c_float), ("hit_terminates", ctypes.c_int32), ("hit_reward", ctypes.c_float),
                ("prox_margin", ctypes.c_float), ("prox_weight", ctypes.c_float), ("n_rays", ctypes.c_int32), ("ray_frame", ctypes.c_int32),
                ("max_range", ctypes.c_float)]


class GpdCtbrTask(ctypes.Structure):
    """mirror of `struct GpdCtbrTask` (gpd_rollout_ctbr_task: the affine map from a normalised action to the command)"""
    _fields_ = [("act_scale", ctypes.c_float * 4), ("act_bias", ctypes.c_float * 4), ("normalized", ctypes.c_int32), ("pad_", ctypes.c_int32 * 3)]


#: `mode` of gpd_rollout_ctbr (GPD_CTBR_CMD / GPD_CTBR_POS)
CTBR_MODES = {"cmd": 0, "pos": 1}

#: floats of MRAC state per controller (GPD_MRAC_STATE): Kx [12][4] | Kr [4][4] | Xm [12]
MRAC_STATE = 76

DEBUG_LIB_PATH = os.path.join(CSRC, "libgpd_debug.so")


def build(force: bool = False, verbose: bool = False, debug: bool = False) -> str:
    """Compile the five units of csrc/ -> csrc/libgpd.so for gfx950 (side by side).  Returns the library path.
    `debug=True`: the debug-bounds build (-DGPD_DEBUG_BOUNDS, include/gpd.h `gpd_debug_status`) -> csrc/libgpd_debug.so; use it by
    setting GPD_LIB to that path before the package is imported."""
    srcs = [os.path.join(CSRC, u) for u, _ in UNITS]
    hdr = os.path.join(INCLUDE, "gpd.h")
    LIB_PATH = DEBUG_LIB_PATH if debug else globals()["LIB_PATH"]
    if not force and os.path.exists(LIB_PATH):
        newest = max([os.path.getmtime(f) for f in srcs] + [os.path.getmtime(hdr)] + [os.path.getmtime(os.path.join(CSRC, h)) for h in HEADERS])
        if os.path.getmtime(LIB_PATH) >= newest:
            return LIB_PATH
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    objs, procs = [], []
    for (unit, extra), src in zip(UNITS, srcs):          # the units compile side by side
        obj = os.path.join(CSRC, unit.replace(".hip", ".dbg.o" if debug else ".o"))
        cmd = [hipcc] + COMMON_FLAGS + extra + (["-DGPD_DEBUG_BOUNDS"] if debug else []) + ["-I", INCLUDE, "-c", src, "-o", obj]
        if verbose:
            print(" ".join(cmd))
        procs.append((cmd, subprocess.Popen(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)))
        objs.append(obj)
    for cmd, pr in procs:
        out, _ = pr.communicate()
        if pr.returncode != 0:
            raise GpdError("hipcc failed: " + " ".join(cmd) + "\n" + out)
    cmd = [hipcc, "--offload-arch=gfx950", "-shared", "-fPIC"] + objs + ["-o", LIB_PATH]
    if verbose:
        print(" ".join(cmd))
    res = subprocess.run(cmd, capture_output=True, text=True)
    if res.returncode != 0:
        raise GpdError("hipcc (link) failed:\n" + res.stdout + res.stderr)
    for o in objs:
        os.remove(o)
    return LIB_PATH


_lib = None

_P = ctypes.c_void_p
_SIGNATURES = {
    "gpd_abi_version": (ctypes.c_int, []),
    "gpd_last_error": (ctypes.c_char_p, []),
    "gpd_struct_sizes": (None, [ctypes.POINTER(ctypes.c_int32)]),
    "gpd_step": (ctypes.c_int, [ctypes.POINTER(GpdParams), ctypes.POINTER(GpdState), ctypes.POINTER(GpdStepCfg),
                                _P, _P, _P, _P, _P, _P, _P, _P, _P]),
    "gpd_step_sync": (ctypes.c_int, [ctypes.POINTER(GpdParams), ctypes.POINTER(GpdState), ctypes.POINTER(GpdStepCfg),
                                     _P, _P, _P, _P, _P, _P, _P, _P, _P]),
    "gpd_rollout": (ctypes.c_int, [ctypes.POINTER(GpdParams), ctypes.POINTER(GpdState), ctypes.POINTER(GpdStepCfg),
                                   ctypes.c_int32, _P, ctypes.c_int64, _P, _P, _P, ctypes.c_int64, _P, _P, _P,
                                   ctypes.c_int64, _P, _P]),
    "gpd_rollout_history": (ctypes.c_int, [ctypes.POINTER(GpdParams), ctypes.POINTER(GpdState), ctypes.POINTER(GpdStepCfg),
                                           ctypes.c_int32, _P, ctypes.c_int64, _P, _P, _P, ctypes.c_int64, _P, _P, _P,
                                           ctypes.c_int64, _P]),
    "gpd_plant_derive": (ctypes.c_int, [ctypes.POINTER(GpdParams), _P, _P, ctypes.c_int32, ctypes.c_int32, ctypes.c_int64, _P, _P]),
    "gpd_rollout_plant": (ctypes.c_int, [ctypes.POINTER(GpdParams), ctypes.POINTER(GpdState), ctypes.POINTER(GpdStepCfg),
                                         ctypes.c_int32, _P, ctypes.c_int64, _P, _P, _P, ctypes.c_int64, _P, _P, _P,
                                         ctypes.c_int64, _P, _P, _P]),
    "gpd_rollout_policy": (ctypes.c_int, [ctypes.POINTER(GpdParams), ctypes.POINTER(GpdState), ctypes.POINTER(GpdStepCfg), _P,
                                          ctypes.c_int32, _P, _P, _P, _P, _P, ctypes.c_int64, _P, _P, _P, ctypes.c_int64, _P,
                                          ctypes.POINTER(ctypes.c_float), _P, _P, _P]),
    "gpd_hist_rows": (ctypes.c_int, [ctypes.POINTER(GpdState), ctypes.c_int32, ctypes.c_int32, ctypes.c_int32, _P, _P, _P]),
    "gpd_full_obs": (ctypes.c_int, [ctypes.POINTER(GpdState), ctypes.c_int32, ctypes.c_int32, ctypes.c_int32, ctypes.c_int32, _P,
                                    ctypes.c_int64, _P, ctypes.c_int64, _P, ctypes.c_int64, _P]),
    "gpd_downwash_global": (ctypes.c_int, [ctypes.POINTER(GpdParams), _P, ctypes.c_int64, ctypes.c_int32, ctypes.c_float,
                                           ctypes.c_float, ctypes.c_float, ctypes.c_int32, ctypes.c_int32, ctypes.c_float,
                                           ctypes.c_float, ctypes.c_int32, _P, _P, _P, _P, _P, _P, ctypes.POINTER(GpdState), _P, _P, _P]),
    "gpd_sizeof_swarm": (ctypes.c_int, []),
    "gpd_swarm_step": (ctypes.c_int, [ctypes.POINTER(GpdParams), ctypes.POINTER(GpdState), ctypes.POINTER(GpdStepCfg),
                                      ctypes.POINTER(GpdSwarm), _P, _P, _P, _P]),
    "gpd_swarm_pack": (ctypes.c_int, [ctypes.POINTER(GpdState), ctypes.POINTER(GpdSwarm), _P, _P, _P]),
    "gpd_swarm_bin": (ctypes.c_int, [ctypes.POINTER(GpdSwarm), _P]),
    "gpd_swarm_forces": (ctypes.c_int, [ctypes.POINTER(GpdParams), ctypes.POINTER(GpdSwarm), ctypes.c_int32, _P]),
    "gpd_neighbors": (ctypes.c_int, [_P, ctypes.c_int32, ctypes.c_int32, ctypes.c_int32, ctypes.c_float, ctypes.c_int32, ctypes.c_int32,
                                     ctypes.c_float, ctypes.c_float, ctypes.c_float, ctypes.c_float, ctypes.c_float, _P, _P, _P, _P, _P, _P,
                                     _P, _P, _P, _P]),
    "gpd_obstacles": (ctypes.c_int, [_P, _P, ctypes.c_int32, ctypes.c_int32, _P, ctypes.c_int32, ctypes.c_int64, ctypes.c_float, _P, _P, _P,
                                     _P, ctypes.c_int32, ctypes.c_int32, ctypes.c_float, _P, _P, _P]),
    "gpd_sizeof_obst_task": (ctypes.c_int, [ctypes.POINTER(ctypes.c_int32)]),
    "gpd_rollout_obst": (ctypes.c_int, [ctypes.POINTER(GpdParams), ctypes.POINTER(GpdState), ctypes.POINTER(GpdStepCfg), ctypes.POINTER(GpdObstTask),
                                        ctypes.c_int32, _P, ctypes.c_int64, _P, _P, _P, ctypes.c_int32, ctypes.c_int64, _P, _P, ctypes.c_int64,
                                        ctypes.c_int64, _P, _P, _P, _P, ctypes.c_int64, _P]),
    "gpd_mppi": (ctypes.c_int, [ctypes.POINTER(GpdParams), ctypes.POINTER(GpdState), ctypes.POINTER(GpdStepCfg), ctypes.POINTER(GpdMppi), _P,
                                ctypes.c_int64, _P, ctypes.c_int64, _P, ctypes.c_int32, ctypes.c_int64, _P, _P, _P, _P]),
    "gpd_mppi_ctbr": (ctypes.c_int, [ctypes.POINTER(GpdParams), ctypes.POINTER(GpdCtbr), ctypes.POINTER(GpdState), ctypes.POINTER(GpdStepCfg),
                                     ctypes.POINTER(GpdMppi), _P, ctypes.c_int64, _P, ctypes.c_int64, _P, ctypes.c_int32, ctypes.c_int64, _P, _P, _P, _P]),
    "gpd_mppi_peers": (ctypes.c_int, [ctypes.POINTER(GpdParams), ctypes.POINTER(GpdCtbr), ctypes.POINTER(GpdState), ctypes.POINTER(GpdStepCfg),
                                      ctypes.POINTER(GpdMppi), ctypes.POINTER(GpdMppiPeers), _P, ctypes.c_int64, _P, ctypes.c_int64, _P, ctypes.c_int32,
                                      ctypes.c_int64, _P, _P, _P, _P]),
    "gpd_mppi_plant": (ctypes.c_int, [ctypes.POINTER(GpdParams), ctypes.POINTER(GpdCtbr), ctypes.POINTER(GpdState), ctypes.POINTER(GpdStepCfg),
                                      ctypes.POINTER(GpdMppi), _P, _P, ctypes.c_int64, _P, ctypes.c_int64, _P, ctypes.c_int32, ctypes.c_int64,
                                      _P, _P, _P, _P]),
    "gpd_reset": (ctypes.c_int, [ctypes.POINTER(GpdState), _P, ctypes.c_int32, _P, ctypes.c_int32, ctypes.c_int32,
                                 ctypes.c_int32, _P, _P]),
    "gpd_pid": (ctypes.c_int, [ctypes.POINTER(GpdParams), _P, ctypes.c_int64, ctypes.c_float, _P, _P, _P, _P, _P, _P,
                               _P, _P, _P, _P, ctypes.c_int32, _P]),
    "gpd_pid_sync": (ctypes.c_int, [ctypes.POINTER(GpdParams), _P, ctypes.c_int64, ctypes.c_float, _P, _P, _P, _P, _P, _P,
                                    _P, _P, _P, _P, ctypes.c_int32, _P]),
    "gpd_sizeof_mrac": (ctypes.c_int, [ctypes.POINTER(ctypes.c_int32)]),
    "gpd_mrac": (ctypes.c_int, [ctypes.POINTER(GpdMrac), _P, _P, ctypes.c_int64, ctypes.c_float, _P, _P, _P, _P, _P, _P, _P, _P, _P, _P, _P,
                                ctypes.c_int32, _P]),
    "gpd_mrac_reset": (ctypes.c_int, [_P, _P, ctypes.c_int64, ctypes.POINTER(GpdMrac), _P, ctypes.c_int32, ctypes.c_int32, _P]),
    "gpd_rollout_mrac": (ctypes.c_int, [ctypes.POINTER(GpdParams), ctypes.POINTER(GpdMrac), ctypes.POINTER(GpdState),
                                        ctypes.POINTER(GpdStepCfg), _P, _P, ctypes.c_int64, _P, ctypes.c_int64, _P, _P, _P, ctypes.c_int64,
                                        ctypes.c_int32, _P]),
    "gpd_sizeof_ctbr": (ctypes.c_int, [ctypes.POINTER(ctypes.c_int32)]),
    "gpd_ctbr": (ctypes.c_int, [ctypes.POINTER(GpdCtbr), _P, _P, _P, _P, _P, _P, ctypes.c_int32, _P]),
    "gpd_rollout_ctbr": (ctypes.c_int, [ctypes.POINTER(GpdParams), ctypes.POINTER(GpdCtbr), ctypes.POINTER(GpdState), ctypes.POINTER(GpdStepCfg),
                                        ctypes.c_int32, _P, ctypes.c_int64, _P, _P, ctypes.c_int64, _P, ctypes.c_int32, _P]),
    "gpd_task_eval": (ctypes.c_int, [ctypes.POINTER(GpdStepCfg), _P, _P, _P, _P, _P, _P, _P]),
    "gpd_sizeof_ctbr_task": (ctypes.c_int, [ctypes.POINTER(ctypes.c_int32)]),
    "gpd_rollout_ctbr_task": (ctypes.c_int, [ctypes.POINTER(GpdParams), ctypes.POINTER(GpdCtbr), ctypes.POINTER(GpdState), ctypes.POINTER(GpdStepCfg),
                                             ctypes.POINTER(GpdCtbrTask), ctypes.c_int32, _P, ctypes.c_int64, _P, _P, _P, _P, _P, ctypes.c_int64, _P, _P, _P,
                                             ctypes.c_int64, _P, _P]),
    "gpd_state_vectors": (ctypes.c_int, [ctypes.POINTER(GpdState), _P, _P, ctypes.c_int32, _P]),
    "gpd_comm_unique_id": (ctypes.c_int, [ctypes.POINTER(ctypes.c_uint8)]),
    "gpd_comm_init": (ctypes.c_int, [ctypes.POINTER(ctypes.c_void_p), ctypes.POINTER(ctypes.c_uint8), ctypes.c_int32,
                                     ctypes.c_int32]),
    "gpd_comm_count": (ctypes.c_int, [_P, ctypes.POINTER(ctypes.c_int32)]),
    "gpd_comm_destroy": (ctypes.c_int, [_P]),
    "gpd_allgather_obs": (ctypes.c_int, [_P, _P, _P, ctypes.c_size_t, _P]),
    "gpd_p2p_group": (ctypes.c_int, [_P, ctypes.POINTER(GpdP2P), ctypes.c_int32, ctypes.POINTER(GpdP2P), ctypes.c_int32, _P]),
    "gpd_debug_status": (ctypes.c_int, [ctypes.POINTER(ctypes.c_uint32), ctypes.c_int32, _P]),
    "gpd_clock_probe": (ctypes.c_int, [ctypes.POINTER(ctypes.c_double), ctypes.POINTER(ctypes.c_double), _P]),
    # the differentiable rollout (diff.py): the taped forward, its reverse sweep, the tape's size
    "gpd_rollout_tape_floats": (ctypes.c_int, [ctypes.POINTER(GpdStepCfg), ctypes.c_int32, ctypes.c_int64, ctypes.POINTER(ctypes.c_int64)]),
    "gpd_rollout_tape": (ctypes.c_int, [ctypes.POINTER(GpdParams), ctypes.POINTER(GpdState), ctypes.POINTER(GpdStepCfg), ctypes.c_int32, _P,
                                        ctypes.c_int64, _P, _P, ctypes.c_int64, _P, _P, _P, ctypes.c_int64, _P, _P, _P]),
    "gpd_rollout_vjp": (ctypes.c_int, [ctypes.POINTER(GpdParams), ctypes.POINTER(GpdStepCfg), ctypes.c_int64, ctypes.c_int32, _P,
                                       ctypes.c_int64, _P, _P, _P, _P, ctypes.c_int64, _P, ctypes.c_int64, _P, _P, _P]),
    # ... and the gradients with respect to the plant: the sweep that also returns the plant rows' cotangents, rows -> scale factors
    "gpd_rollout_vjp_plant": (ctypes.c_int, [ctypes.POINTER(GpdParams), ctypes.POINTER(GpdStepCfg), ctypes.c_int64, ctypes.c_int32, _P,
                                             ctypes.c_int64, _P, _P, _P, _P, ctypes.c_int64, _P, ctypes.c_int64, _P, _P, _P, _P]),
    "gpd_plant_derive_vjp": (ctypes.c_int, [ctypes.POINTER(GpdParams), _P, _P, ctypes.c_int32, ctypes.c_int64, _P, _P]),
    # ... and through the DSLPID loop: the members as a differentiable input and output, the gains' cotangents
    "gpd_rollout_tape_pid_floats": (ctypes.c_int, [ctypes.POINTER(GpdStepCfg), ctypes.c_int32, ctypes.c_int64, ctypes.POINTER(ctypes.c_int64)]),
    "gpd_rollout_tape_pid": (ctypes.c_int, [ctypes.POINTER(GpdParams), ctypes.POINTER(GpdState), ctypes.POINTER(GpdStepCfg), ctypes.c_int32, _P,
                                            ctypes.c_int64, _P, _P, ctypes.c_int64, _P, _P, _P, ctypes.c_int64, _P, _P]),
    "gpd_rollout_vjp_pid": (ctypes.c_int, [ctypes.POINTER(GpdParams), ctypes.POINTER(GpdStepCfg), ctypes.c_int64, ctypes.c_int32, _P,
                                           ctypes.c_int64, _P, _P, _P, ctypes.c_int64, _P, ctypes.c_int64, _P, _P, _P, _P, _P]),
    # ... and through the thrust-and-body-rate loop: gpd_rollout_ctbr's arguments plus the tape; the 12 gains' cotangents
    "gpd_rollout_tape_ctbr_floats": (ctypes.c_int, [ctypes.POINTER(GpdStepCfg), ctypes.c_int32, ctypes.c_int64, ctypes.POINTER(ctypes.c_int64)]),
    "gpd_rollout_tape_ctbr": (ctypes.c_int, [ctypes.POINTER(GpdParams), ctypes.POINTER(GpdCtbr), ctypes.POINTER(GpdState), ctypes.POINTER(GpdStepCfg),
                                             ctypes.c_int32, _P, ctypes.c_int64, _P, _P, ctypes.c_int64, _P, ctypes.c_int32, _P, _P]),
    "gpd_rollout_vjp_ctbr": (ctypes.c_int, [ctypes.POINTER(GpdParams), ctypes.POINTER(GpdCtbr), ctypes.POINTER(GpdStepCfg), ctypes.c_int64,
                                            ctypes.c_int32, ctypes.c_int32, _P, ctypes.c_int64, _P, _P, _P, ctypes.c_int64, _P, _P, _P, _P]),
}
COMM_ID_BYTES = 128
GPD_EINVAL, GPD_ERANGE, GPD_ENOTSUP = -1, -2, -3

#: the plant path (include/gpd.h): the nine per-drone scale factors, in the order of GPD_SCALE_* ...
SCALE_FIELDS = ("mass", "ixx", "iyy", "izz", "kf", "km", "drag_xy", "drag_z", "gnd_eff")
#: ... and the derived plant rows, in the order of GPD_PLANT_* (the GpdParams field each row replaces; the last two are new)
PLANT_ROW_FIELDS = ("M", "inv_M", "KF", "GRAVITY", "J[0]", "J[1]", "J[2]", "J_INV[0]", "J_INV[1]", "J_INV[2]", "km_over_kf",
                    "gnd_eff_coeff", "drag_coeff[0]", "drag_coeff[1]", "drag_coeff[2]", "hover_thrust", "hover_resid", "norm_thrust",
                    "norm_gap")
PLANT_ROWS = len(PLANT_ROW_FIELDS)


def lib() -> ctypes.CDLL:
    """Load (once) and verify the shared library.  Raises GpdError when it is absent or stale."""
    global _lib
    if _lib is not None:
        return _lib
    path = os.environ.get("GPD_LIB", LIB_PATH)     # GPD_LIB: A/B-test another build of the same ABI
    if not os.path.exists(path):
        raise GpdError(f"{path} not found: the HIP extension has not been built "
                       "(run `python -c 'import __graft_entry__ as g; g.build()'`). "
                       "There is no CPU fallback for the simulator's hot path.")
    try:
        L = ctypes.CDLL(path)
    except OSError as e:
        raise GpdError(f"cannot load {path}: {e}") from e
    for name, (res, args) in _SIGNATURES.items():
        try:
            fn = getattr(L, name)
        except AttributeError as e:
            raise GpdError(f"{path} does not export {name}") from e
        fn.restype = res
        fn.argtypes = args
    if L.gpd_abi_version() != ABI_VERSION:
        raise GpdError(f"libgpd ABI {L.gpd_abi_version()} != binding ABI {ABI_VERSION}; rebuild")
    sizes = (ctypes.c_int32 * 3)()
    L.gpd_struct_sizes(sizes)
    want = (ctypes.sizeof(GpdParams), ctypes.sizeof(GpdState), ctypes.sizeof(GpdStepCfg))
    if tuple(sizes) != want:
        raise GpdError(f"struct layout mismatch: library {tuple(sizes)} vs binding {want}")
    if L.gpd_sizeof_swarm() != ctypes.sizeof(GpdSwarm):
        raise GpdError(f"struct layout mismatch: GpdSwarm is {L.gpd_sizeof_swarm()} bytes in the library, {ctypes.sizeof(GpdSwarm)} in the binding")
    mrac_size = ctypes.c_int32(0)
    if L.gpd_sizeof_mrac(ctypes.byref(mrac_size)) != 0 or mrac_size.value != ctypes.sizeof(GpdMrac):
        raise GpdError(f"struct layout mismatch: GpdMrac is {mrac_size.value} bytes in the library, {ctypes.sizeof(GpdMrac)} in the binding")
    ctbr_size = ctypes.c_int32(0)
    if L.gpd_sizeof_ctbr(ctypes.byref(ctbr_size)) != 0 or ctbr_size.value != ctypes.sizeof(GpdCtbr):
        raise GpdError(f"struct layout mismatch: GpdCtbr is {ctbr_size.value} bytes in the library, {ctypes.sizeof(GpdCtbr)} in the binding")
    obst_size = ctypes.c_int32(0)
    if L.gpd_sizeof_obst_task(ctypes.byref(obst_size)) != 0 or obst_size.value != ctypes.sizeof(GpdObstTask):
        raise GpdError(f"struct layout mismatch: GpdObstTask is {obst_size.value} bytes in the library, {ctypes.sizeof(GpdObstTask)} in the binding")
    task_size = ctypes.c_int32(0)
    if L.gpd_sizeof_ctbr_task(ctypes.byref(task_size)) != 0 or task_size.value != ctypes.sizeof(GpdCtbrTask):
        raise GpdError(f"struct layout mismatch: GpdCtbrTask is {task_size.value} bytes in the library, {ctypes.sizeof(GpdCtbrTask)} in the binding")
    _lib = L
    return L


def check(rc: int, what: str):
    if rc != 0:
        msg = lib().gpd_last_error().decode("utf-8", "replace")
        raise GpdError(f"{what} failed (code {rc}): {msg}")


def exported_symbols():
    return list(_SIGNATURES)


# ---- the one way in: every launch off the hot paths is one `call(...)` line; the hot paths pre-build their tuples with `as_c` ----
#: `stream` of `call` for the entries that take none (gpd_comm_*, gpd_sizeof_mrac ...)
NO_STREAM = object()
_get_raw_stream = getattr(getattr(torch, "_C", None), "_cuda_getCurrentRawStream", None)


def raw_stream(device) -> int:
    """hipStream_t of torch's current stream on `device` (the accessor torch's own compiled kernels use: no Stream object per call)"""
    if _get_raw_stream is not None and device.index is not None:
        return _get_raw_stream(device.index)
    return torch.cuda.current_stream(device).cuda_stream


_NO_GUARD = contextlib.nullcontext()
_Tensor = getattr(torch, "Tensor", None)
#: what `as_c` has nothing to do for: NULL, numbers, and the two kinds of object it returns itself (a pre-built tuple passes through)
_AS_IS = frozenset((type(None), int, float, bool, ctypes.c_void_p, type(ctypes.byref(ctypes.c_int()))))


def device_guard(device):
    """the device guard, or nothing when `device` (None: whichever) is the current one already"""
    if device is None or device.index is None or device.index == torch.cuda.current_device():
        return _NO_GUARD
    return torch.cuda.device(device)


def as_c(x):
    """One argument as ctypes takes it: a tensor -> its address, a struct -> a reference to it (explicitly: an entry that takes a
    struct through a plain `void *`, like gpd_rollout_policy's policy, gets no automatic by-reference passing from ctypes);
    None (NULL), numbers and ready-made ctypes objects as they are."""
    kind = type(x)          # (exact types first: `isinstance(3, torch.Tensor)` costs more than the whole function does this way)
    if kind is _Tensor:
        return ctypes.c_void_p(x.data_ptr())
    if kind in _AS_IS:
        return x
    if isinstance(x, ctypes.Structure):
        return ctypes.byref(x)
    if isinstance(x, _Tensor):      # (a subclass: a Parameter, engine.KinRows)
        return ctypes.c_void_p(x.data_ptr())
    return x


def call(name: str, device, stream, *args, allow=(), what: str = None) -> int:
    """`lib().<name>(*args, stream)` with `device` current (None: whatever is), the arguments converted by `as_c`; raises GpdError
    (naming `what`, by default the entry) unless the entry returns 0 or a code in `allow`, which is returned."""
    fn = getattr(lib(), name)
    argv = [a if type(a) in _AS_IS else as_c(a) for a in args]
    if stream is not NO_STREAM:
        argv.append(stream)
    with device_guard(device):
        rc = fn(*argv)
    if rc and rc not in allow:
        check(rc, what or name)
    return rc
