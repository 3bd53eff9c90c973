"""The differentiable rollout: analytic gradients through the K-step kernel (include/gpd.h `gpd_rollout_tape` / `gpd_rollout_vjp`,
csrc/diff_kernels.inc).

    obs12, reward, kin_K, terminated, truncated = core.rollout_diff(actions)          # actions [K, N, A], requires_grad
    loss(obs12, reward, kin_K).backward()                                             # one reverse-sweep launch

The forward is the rollout kernel's own arithmetic (bit for bit `SimCore.rollout`) plus a tape of 52 B per drone-step; the backward is
a hand-written reverse sweep on the device, one lane per drone, no atomics (two calls give the same bits).  Differentiable inputs: the
actions and the initial kinematic state (the `[13 * ld]` plane layout of `SimCore.kin_store`; `pack_kin` / `unpack_kin` convert).
Feeding `kin_K` of one call into `kin0` of the next chains the graph: K = 1 is the closed-loop primitive, with a torch policy between
steps.  Supported: single-drone aviaries, no task or the hover task, the four RPM action types, no add-on physics or drag, with or
without a plant table, no auto-reset; everything else raises `GpdError` with the library's message.  First derivatives only.

    obs12, *_ = core.rollout_diff(actions, plant_scales=scales)                       # scales [9, E] or [9, E, 1], requires_grad
    loss(obs12).backward()                                                            # scales.grad: d loss / d (the nine scale factors)

With `plant_scales=` the per-drone plant (`SimCore.set_plant`) is the third differentiable input: the call installs the scales as the
core's plant table, and the backward is `gpd_rollout_vjp_plant` (the same sweep, which also sums the cotangents of the plant rows it
reads) followed by `gpd_plant_derive_vjp` (rows -> scale factors).  System identification and calibration: examples/sysid.py.

    obs12, reward, kin_K, pid_K, *_ = core.rollout_diff_pid(actions, pid_gains=gains)     # a PID / VEL / ONE_D_PID core; gains [6, 3]
    loss(obs12).backward()                                                                # actions.grad, gains.grad

The three action types that close the loop in the kernel go through `rollout_diff_pid` (`gpd_rollout_tape_pid` /
`gpd_rollout_vjp_pid`): the nine controller members (`pack_pid` / `unpack_pid`) are a differentiable input
and output next to the kinematic state, and the 18 gains of the cascaded PID receive a gradient.  Tuning the controller by
back-propagation through the flight: examples/tune_pid.py.

    obs12, kin_K = core.rollout_diff_ctbr(ctrl, cmd, gains=gains)                         # cmd [K, N, 4]: thrust | body rates; gains [4, 3]
    loss(obs12).backward()                                                                # cmd.grad, gains.grad

Thrust and body-rate commands -- `SimCore.rollout_ctbr`'s flight, a rate loop inside every sub-step -- go through
`rollout_diff_ctbr` (`gpd_rollout_tape_ctbr` / `gpd_rollout_vjp_ctbr`): commands (`mode="cmd"`) or target rows
through the reference's outer loop (`mode="pos"`), the initial state and the controller's 12 gains receive gradients.  Policy
gradients through the physics on the action space of agile flight: examples/apg_ctbr.py.
"""
import ctypes

import torch
from torch.autograd.function import once_differentiable

from . import _native


def pack_kin(pos, quat, vel, rates, ld: int = None):
    """(pos [N,3], quat [N,4] xyzw, vel [N,3], body rates [N,3]) -> the `[13 * ld]` plane layout of `GpdState.kin` (ld: N rounded up to
    64 by default; the padding is zero).  Differentiable torch code."""
    n = pos.shape[0]
    ld = (n + 63) // 64 * 64 if ld is None else int(ld)
    P = torch.cat([pos, rates[:, 0:1]], dim=1)
    V = torch.cat([vel, rates[:, 1:2]], dim=1)
    pad4 = pos.new_zeros((ld - n, 4))
    return torch.cat([torch.cat([P, pad4]).reshape(-1), torch.cat([quat, pad4]).reshape(-1), torch.cat([V, pad4]).reshape(-1),
                      rates[:, 2], pos.new_zeros(ld - n)])


def unpack_kin(kin, n: int = None):
    """the `[13 * ld]` plane layout -> (pos [n,3], quat [n,4], vel [n,3], body rates [n,3]) (n: ld by default).  Differentiable."""
    ld = kin.numel() // 13
    n = ld if n is None else int(n)
    P, Q, V, W = kin[:4 * ld].view(ld, 4)[:n], kin[4 * ld:8 * ld].view(ld, 4)[:n], kin[8 * ld:12 * ld].view(ld, 4)[:n], kin[12 * ld:][:n]
    return P[:, :3], Q, V[:, :3], torch.stack([P[:, 3], V[:, 3], W], dim=1)


def tape_floats(core, K: int) -> int:
    """floats of the tape of a K-step call on `core` (`gpd_rollout_tape_floats`); raises GpdError for an unsupported configuration"""
    out = ctypes.c_int64(0)
    _native.call("gpd_rollout_tape_floats", None, _native.NO_STREAM, core._cfg, int(K), core.ld, ctypes.byref(out))
    return out.value


def tape_forward(core, K, actions, a_stride, obs, rew, term, trunc, tape):
    """one `gpd_rollout_tape` launch on the core's params, state, cfg, target and plant rows (None: the nominal airframe): K steps of
    `actions` (`a_stride` floats apart, 0: one shared block) into `obs [K,N,12]`, `rew`, `term`, `trunc [K,E]` and `tape`"""
    _native.call("gpd_rollout_tape", core.device, core._stream(), core._params, core._state, core._cfg, K, actions, a_stride, core.target,
                 obs, core.N * 12, rew, term, trunc, core.E, core.plant_rows, tape)


#: `target` / `plant` of `sweep`: the core's own, as it stands now (None is an answer of its own: no target, the nominal airframe)
OWN = object()


def sweep(core, K, actions, a_stride, tape, g_obs, g_rew, g_kin, g_act, target=OWN, plant=OWN, g_rows=None):
    """one reverse-sweep launch over `tape`: `gpd_rollout_vjp`, or -- with `g_rows [19, ld]` to receive the plant rows' cotangents --
    `gpd_rollout_vjp_plant`.  `g_obs` / `g_rew`: None = zeros; `g_kin` is read and overwritten, `g_act [K,N,A]` written.  `target`
    and `plant` default to the core's own; the backward passes the ones its forward flew (None included: a plant installed since
    must not reach a tape that was recorded without one)."""
    entry, rows = ("gpd_rollout_vjp", ()) if g_rows is None else ("gpd_rollout_vjp_plant", (g_rows,))
    _native.call(entry, core.device, core._stream(), core._params, core._cfg, core.ld, K, actions, a_stride,
                 core.target if target is OWN else target, core.plant_rows if plant is OWN else plant, tape, g_obs, core.N * 12, g_rew,
                 core.E, g_kin, g_act, *rows)


def derive_vjp(core, scales, g_rows, g_scales):
    """`gpd_plant_derive_vjp`: the plant rows' cotangents `g_rows [19, ld]` at `scales [9, ld]` -> `g_scales [9, ld]` (drones 0 .. N-1)"""
    _native.call("gpd_plant_derive_vjp", core.device, core._stream(), core._params, scales, g_rows, core.N, core.ld, g_scales)


# ---- what the two autograd functions (RolloutDiff, RolloutDiffPid) share ---------------------------------------------------------------
def _state0(core, x, own, name, layout):
    """`kin0` / `pid0` of a call: None (the core's `own` block, `rows x ld`) or a tensor of as many elements, as float32 in its shape"""
    if x is None:
        return own.detach()
    rows = own.numel() // core.ld
    if x.numel() != own.numel():
        raise ValueError(f"{name} has {x.numel()} elements, expected {rows} x ld = {rows * core.ld} ({layout})")
    return x.to(device=core.device, dtype=torch.float32).reshape(own.shape).contiguous()


def _outputs(core, K, size):
    """fresh `(obs [K,N,12], rew [K,E], term [K,E], trunc [K,E], tape [size])` for a taped forward of K steps"""
    dev, E = core.device, core.E
    return (torch.empty((K, core.N, 12), dtype=torch.float32, device=dev), torch.empty((K, E), dtype=torch.float32, device=dev),
            torch.empty((K, E), dtype=torch.bool, device=dev), torch.empty((K, E), dtype=torch.bool, device=dev),
            torch.empty((size,), dtype=torch.float32, device=dev))


def _cot(g, like=None):
    """a cotangent as the sweeps take it: float32 and contiguous.  Of obs12 / reward (`like` None): None stays None, NULL = zeros; of a
    state block: a COPY (the sweep overwrites it), None = zeros like `like`"""
    if like is None:
        return None if g is None else g.to(torch.float32).contiguous()
    return torch.zeros_like(like) if g is None else g.to(torch.float32).clone(memory_format=torch.contiguous_format)


def _action_grad(g_act, a_stride, actions):
    """`g_act [K,N,A]` in the shape of `actions`; a shared action block's gradient is the sum over the steps"""
    return (g_act.sum(dim=0) if a_stride == 0 else g_act).view(actions.shape)


class RolloutDiff(torch.autograd.Function):
    """forward: `gpd_rollout_tape` from `kin0` (copied into the core's state first); backward: `gpd_rollout_vjp`, or -- when
    `plant_scales` (the scales `rollout_diff` has just installed with `set_plant`) asks for a gradient -- `gpd_rollout_vjp_plant`
    and `gpd_plant_derive_vjp`"""

    @staticmethod
    def forward(ctx, core, kin0, actions, K, a_stride, plant_scales=None, own_plant=False):
        size = tape_floats(core, K)                            # (also the configuration check, before anything is touched)
        if kin0.data_ptr() != core.kin_store.data_ptr():
            core.kin_store.copy_(kin0)
        obs, rew, term, trunc, tape = _outputs(core, K, size)
        core.state_version += 1
        tape_forward(core, K, actions, a_stride, obs, rew, term, trunc, tape)
        kin_k = core.kin_store.clone()
        core._publish_latest(obs, rew, term, trunc, K)          # (the core's latest-step tensors follow its state, as after rollout())
        ctx.core, ctx.K, ctx.a_stride, ctx.plant = core, K, a_stride, core.plant_rows
        ctx.target = core.target
        ctx.scales = None
        if own_plant:          # (copies: the next plant_scales= rewrites the core's tables in place; the backward needs the ones this call flew)
            ctx.plant = core.plant_rows.clone()
            if plant_scales is not None and plant_scales.requires_grad:
                ctx.scales, ctx.scales_shape = core.plant_scales.clone(), plant_scales.shape
        ctx.save_for_backward(actions, tape)
        ctx.mark_non_differentiable(term, trunc)
        ctx.set_materialize_grads(False)                       # (an output nobody differentiates arrives as None: NULL = zeros)
        return obs, rew, kin_k, term, trunc

    @staticmethod
    @once_differentiable
    def backward(ctx, g_obs, g_rew, g_kin, _g_term, _g_trunc):
        core, K = ctx.core, ctx.K
        actions, tape = ctx.saved_tensors
        dev, N = core.device, core.N
        g_kin = _cot(g_kin, core.kin_store)
        g_act = torch.empty((K, N, core.A), dtype=torch.float32, device=dev)
        with_scales = ctx.scales is not None and ctx.needs_input_grad[5]
        g_rows = torch.empty((_native.PLANT_ROWS, core.ld), dtype=torch.float32, device=dev) if with_scales else None     # (both kernels write drones 0 .. N-1)
        sweep(core, K, actions, ctx.a_stride, tape, _cot(g_obs), _cot(g_rew), g_kin, g_act, ctx.target, ctx.plant, g_rows)
        g_scales = None
        if with_scales:
            g_table = torch.empty((len(_native.SCALE_FIELDS), core.ld), dtype=torch.float32, device=dev)
            derive_vjp(core, ctx.scales, g_rows, g_table)
            g_scales = g_table[:, :N].reshape(ctx.scales_shape)
        return None, g_kin, _action_grad(g_act, ctx.a_stride, actions), None, None, g_scales, None


def rollout_diff(core, actions, kin0=None, num_steps: int = None, plant_scales=None):
    """`SimCore.rollout_diff`: K env steps in one launch, differentiable with respect to `actions`, `kin0` and `plant_scales`.

    `actions`: float32 device tensor with K x N x A elements (K leading), or -- with `num_steps=K` -- ONE block of N x A elements
    applied at every step (its gradient is the sum over the steps).  `kin0`: None (start from the core's own state) or a `[13 * ld]`
    tensor in the plane layout (`pack_kin`), copied into the state first.  Returns fresh tensors
    `(obs12 [K,N,12], reward [K,E], kin_K [13*ld], terminated [K,E], truncated [K,E])`; the first three carry gradients.
    `plant_scales`: None (the core's plant, or none, as it stands: a constant) or the scale factors in any form `set_plant` accepts.
    They REPLACE the core's plant table (`set_plant(plant_scales.detach())`, with its validation), the forward then is the one above;
    a float tensor `[9, E]` / `[9, E, 1]` that requires grad receives its gradient in its own shape."""
    actions, K, a_stride = core._action_blocks(actions, num_steps)
    kin0 = _state0(core, kin0, core.kin_store, "kin0", "the plane layout: pack_kin")
    if plant_scales is None:
        return RolloutDiff.apply(core, kin0, actions, K, a_stride)
    tape_floats(core, K)                                       # (the configuration check, before the plant table is touched)
    if isinstance(plant_scales, torch.Tensor):
        plant_scales = plant_scales.to(device=core.device, dtype=torch.float32)
        core.set_plant(plant_scales.detach())
    else:
        core.set_plant(plant_scales)
        plant_scales = None
    return RolloutDiff.apply(core, kin0, actions, K, a_stride, plant_scales, True)


# ---- through the DSLPID loop (include/gpd.h `gpd_rollout_tape_pid` / `gpd_rollout_vjp_pid`, csrc/diff_pid_kernels.inc) ----------------
#: the rows of `pid_gains` [6, 3], in the order of `g_gains [18][ld]` and of the fields of GpdParams
GAIN_FIELDS = ("p_for", "i_for", "d_for", "p_tor", "i_tor", "d_tor")


def pack_pid(int_pos_e, last_rpy, int_rpy_e, ld: int = None):
    """(integral position error [N,3], last rpy [N,3], integral rpy error [N,3]) -> the `[9, ld]` rows of `GpdState.pid` (ld: N rounded
    up to 64 by default; the padding is zero).  Differentiable torch code."""
    n = int_pos_e.shape[0]
    ld = (n + 63) // 64 * 64 if ld is None else int(ld)
    rows = torch.cat([int_pos_e, last_rpy, int_rpy_e], dim=1).t()
    return torch.cat([rows, rows.new_zeros((9, ld - n))], dim=1)


def unpack_pid(pid, n: int = None):
    """the `[9, ld]` rows -> (integral position error [n,3], last rpy [n,3], integral rpy error [n,3]) (n: ld by default).
    Differentiable."""
    pid = pid.view(9, -1)
    n = pid.shape[1] if n is None else int(n)
    rows = pid[:, :n].t()
    return rows[:, 0:3], rows[:, 3:6], rows[:, 6:9]


def gains_of(params):
    """the 18 gains of a `GpdParams` as a float32 CPU tensor `[6, 3]` (rows: GAIN_FIELDS)"""
    return torch.tensor([list(getattr(params, f)) for f in GAIN_FIELDS], dtype=torch.float32)


def params_with_gains(params, gains):
    """a copy of the by-value `GpdParams` whose 18 gains are `gains` ([6, 3], rows: GAIN_FIELDS).  Reads the tensor to the host:
    a synchronisation when it lives on the device."""
    host = gains.detach().to(device="cpu", dtype=torch.float32).reshape(6, 3).tolist()
    out = type(params).from_buffer_copy(params)
    for f, row in zip(GAIN_FIELDS, host):
        setattr(out, f, (ctypes.c_float * 3)(*row))
    return out


def tape_floats_pid(core, K: int) -> int:
    """floats of the tape of a K-step call on `core` (`gpd_rollout_tape_pid_floats`); raises GpdError for an unsupported configuration"""
    out = ctypes.c_int64(0)
    _native.call("gpd_rollout_tape_pid_floats", None, _native.NO_STREAM, core._cfg, int(K), core.ld, ctypes.byref(out))
    return out.value


def tape_forward_pid(core, params, K, actions, a_stride, obs, rew, term, trunc, tape):
    """one `gpd_rollout_tape_pid` launch on the core's state, cfg and target with `params` (the core's own, or a copy with other gains)"""
    _native.call("gpd_rollout_tape_pid", core.device, core._stream(), params, core._state, core._cfg, K, actions, a_stride, core.target,
                 obs, core.N * 12, rew, term, trunc, core.E, tape)


def sweep_pid(core, params, K, actions, a_stride, tape, g_obs, g_rew, g_kin, g_pid, g_act, g_gains=None, target=OWN):
    """one `gpd_rollout_vjp_pid` launch over `tape`: `g_obs` / `g_rew`: None = zeros; `g_kin [13*ld]` and `g_pid [9, ld]` are read and
    overwritten, `g_act [K,N,A]` written, `g_gains [18, ld]` (None: not asked for) written per drone"""
    _native.call("gpd_rollout_vjp_pid", core.device, core._stream(), params, core._cfg, core.ld, K, actions, a_stride,
                 core.target if target is OWN else target, tape, g_obs, core.N * 12, g_rew, core.E, g_kin, g_pid, g_act, g_gains)


class RolloutDiffPid(torch.autograd.Function):
    """forward: `gpd_rollout_tape_pid` from `kin0` / `pid0` (copied into the core's state first); backward: `gpd_rollout_vjp_pid`"""

    @staticmethod
    def forward(ctx, core, kin0, pid0, actions, K, a_stride, pid_gains=None):
        size = tape_floats_pid(core, K)                        # (also the configuration check, before anything is touched)
        params = core._params if pid_gains is None else params_with_gains(core._params, pid_gains)
        if kin0.data_ptr() != core.kin_store.data_ptr():
            core.kin_store.copy_(kin0)
        if pid0.data_ptr() != core.pid.data_ptr():
            core.pid.copy_(pid0.view(9, core.ld))
        obs, rew, term, trunc, tape = _outputs(core, K, size)
        core.state_version += 1
        tape_forward_pid(core, params, K, actions, a_stride, obs, rew, term, trunc, tape)
        kin_k, pid_k = core.kin_store.clone(), core.pid.clone()
        core._publish_latest(obs, rew, term, trunc, K)
        ctx.core, ctx.K, ctx.a_stride, ctx.params, ctx.target = core, K, a_stride, params, core.target
        ctx.with_gains = pid_gains is not None and pid_gains.requires_grad
        ctx.gains_like = None if pid_gains is None else (pid_gains.shape, pid_gains.dtype, pid_gains.device)
        ctx.save_for_backward(actions, tape)
        ctx.mark_non_differentiable(term, trunc)
        ctx.set_materialize_grads(False)                       # (an output nobody differentiates arrives as None: NULL = zeros)
        return obs, rew, kin_k, pid_k, term, trunc

    @staticmethod
    @once_differentiable
    def backward(ctx, g_obs, g_rew, g_kin, g_pid, _g_term, _g_trunc):
        core, K = ctx.core, ctx.K
        actions, tape = ctx.saved_tensors
        dev, N = core.device, core.N
        g_kin, g_pid = _cot(g_kin, core.kin_store), _cot(g_pid, core.pid)
        g_act = torch.empty((K, N, core.A), dtype=torch.float32, device=dev)
        with_gains = ctx.with_gains and ctx.needs_input_grad[6]
        g_rows = torch.zeros((18, core.ld), dtype=torch.float32, device=dev) if with_gains else None     # (the kernel writes drones 0 .. N-1)
        sweep_pid(core, ctx.params, K, actions, ctx.a_stride, tape, _cot(g_obs), _cot(g_rew), g_kin, g_pid, g_act, g_rows, ctx.target)
        g_gains = None
        if with_gains:         # the forward's gains are shared: the sum over drones, in float64 (N terms), in the caller's shape and place
            shape, dtype, device = ctx.gains_like
            g_gains = g_rows[:, :N].sum(dim=1, dtype=torch.float64).reshape(6, 3).to(device=device, dtype=dtype).reshape(shape)
        return None, g_kin, g_pid, _action_grad(g_act, ctx.a_stride, actions), None, None, g_gains


def rollout_diff_pid(core, actions, kin0=None, pid0=None, num_steps: int = None, pid_gains=None):
    """`SimCore.rollout_diff_pid`: K env steps of a PID / VEL / ONE_D_PID core in one launch, differentiable with respect to `actions`,
    `kin0`, `pid0` and `pid_gains`.

    `actions` and `kin0` as in `rollout_diff`.  `pid0`: None (the core's own controller members) or a `[9, ld]` tensor (`pack_pid`),
    copied into the state first.  Returns fresh tensors `(obs12 [K,N,12], reward [K,E], kin_K [13*ld], pid_K [9, ld], terminated [K,E],
    truncated [K,E])`; the first four carry gradients, and `kin_K` / `pid_K` of one call given as `kin0` / `pid0` of the next chain the
    graph.  `pid_gains`: None (the core's gains: constants, no gain gradient) or a `[6, 3]` tensor, rows `GAIN_FIELDS`; it REPLACES
    the gains of the by-value parameter block for this call (the core keeps its own), and -- when it requires grad -- receives the
    gradient summed over drones.  Reading its 18 floats to the host is a SYNCHRONISATION when it lives on the device."""
    actions, K, a_stride = core._action_blocks(actions, num_steps)
    tape_floats_pid(core, K)                                   # (the configuration check, with the library's message, before anything else)
    if core.plant_rows is not None:
        raise _native.GpdError("rollout_diff_pid: the DSLPID sweep flies the nominal airframe only; a per-drone plant table is set "
                               "(set_plant(None) removes it)")
    # what the size query cannot see and gpd_rollout_tape_pid would refuse only after kin0 / pid0 have been copied into the core's state
    if core.pid is None or core._params.pid_kf <= 0.0:
        raise _native.GpdError("rollout_diff_pid: this core has no DSLPID controller (no controller members, or an airframe without one)")
    if core._state.dw_force:
        raise _native.GpdError("rollout_diff_pid: downwash computed outside the kernel (state.dw_force) is not differentiable")
    kin0 = _state0(core, kin0, core.kin_store, "kin0", "the plane layout: pack_kin")
    pid0 = _state0(core, pid0, core.pid, "pid0", "the rows of the controller members: pack_pid")
    if pid_gains is not None:
        if not isinstance(pid_gains, torch.Tensor) or pid_gains.numel() != 18:
            raise ValueError("pid_gains must be a tensor of 6 x 3 gains (rows: p_for, i_for, d_for, p_tor, i_tor, d_tor)")
    return RolloutDiffPid.apply(core, kin0, pid0, actions, K, a_stride, pid_gains)


# ---- through the thrust-and-body-rate loop (include/gpd.h `gpd_rollout_tape_ctbr` / `gpd_rollout_vjp_ctbr`, csrc/diff_ctbr_kernels.inc) ---
#: the rows of `gains` [4, 3], in the order of `g_gains [12][ld]` and of the fields of GpdCtbr
CTBR_GAIN_FIELDS = ("k_p", "k_d", "k_rates", "k_rate")


def ctbr_gains_of(ctbr):
    """the 12 gains of a `GpdCtbr` as a float32 CPU tensor `[4, 3]` (rows: CTBR_GAIN_FIELDS)"""
    return torch.tensor([list(getattr(ctbr, f)) for f in CTBR_GAIN_FIELDS], dtype=torch.float32)


def ctbr_with_gains(ctbr, gains):
    """a copy of the by-value `GpdCtbr` whose 12 gains are `gains` ([4, 3], rows: CTBR_GAIN_FIELDS).  Reads the tensor to the host:
    a synchronisation when it lives on the device."""
    host = gains.detach().to(device="cpu", dtype=torch.float32).reshape(4, 3).tolist()
    out = type(ctbr).from_buffer_copy(ctbr)
    for f, row in zip(CTBR_GAIN_FIELDS, host):
        setattr(out, f, (ctypes.c_float * 3)(*row))
    return out


def tape_floats_ctbr(core, K: int) -> int:
    """floats of the tape of a K-step call on `core` (`gpd_rollout_tape_ctbr_floats`); raises GpdError for an unsupported configuration"""
    out = ctypes.c_int64(0)
    _native.call("gpd_rollout_tape_ctbr_floats", None, _native.NO_STREAM, core._cfg, int(K), core.ld, ctypes.byref(out))
    return out.value


def tape_forward_ctbr(core, ctbr, mode, K, rows, r_stride, obs, tape, cmd=None, plant=OWN):
    """one `gpd_rollout_tape_ctbr` launch on the core's params, state and cfg with the controller `ctbr` (a `GpdCtbr`): K steps of `rows`
    (`r_stride` floats apart, 0: one held block) into `obs [K,N,12]`, `tape` and -- not None -- `cmd`"""
    _native.call("gpd_rollout_tape_ctbr", core.device, core._stream(), core._params, ctbr, core._state, core._cfg, _native.CTBR_MODES[mode],
                 rows, r_stride, core.plant_rows if plant is OWN else plant, obs, core.N * 12, cmd, K, tape)


def sweep_ctbr(core, ctbr, mode, K, rows, r_stride, tape, g_obs, g_kin, g_rows, g_gains=None, plant=OWN):
    """one `gpd_rollout_vjp_ctbr` launch over `tape`: `g_obs`: None = zeros; `g_kin [13*ld]` is read and overwritten, `g_rows [K,N,W]`
    written, `g_gains [12, ld]` (None: not asked for) written per drone"""
    _native.call("gpd_rollout_vjp_ctbr", core.device, core._stream(), core._params, ctbr, core._cfg, core.ld, _native.CTBR_MODES[mode], K,
                 rows, r_stride, core.plant_rows if plant is OWN else plant, tape, g_obs, core.N * 12, g_kin, g_rows, g_gains)


class RolloutDiffCtbr(torch.autograd.Function):
    """forward: `gpd_rollout_tape_ctbr` from `kin0` (copied into the core's state first); backward: `gpd_rollout_vjp_ctbr`"""

    @staticmethod
    def forward(ctx, core, ctbr, kin0, rows, K, r_stride, mode, gains=None):
        size = tape_floats_ctbr(core, K)                       # (also the configuration check, before anything is touched)
        ctbr = ctbr if gains is None else ctbr_with_gains(ctbr, gains)
        if kin0.data_ptr() != core.kin_store.data_ptr():
            core.kin_store.copy_(kin0)
        obs = torch.empty((K, core.N, 12), dtype=torch.float32, device=core.device)
        tape = torch.empty((size,), dtype=torch.float32, device=core.device)
        core.state_version += 1
        tape_forward_ctbr(core, ctbr, mode, K, rows, r_stride, obs, tape)
        kin_k = core.kin_store.clone()
        core.obs12.copy_(obs[K - 1])                           # (the core's latest rows follow its state, as after rollout_ctbr())
        ctx.core, ctx.ctbr, ctx.K, ctx.r_stride, ctx.mode, ctx.plant = core, ctbr, K, r_stride, mode, core.plant_rows
        ctx.with_gains = gains is not None and gains.requires_grad
        ctx.gains_like = None if gains is None else (gains.shape, gains.dtype, gains.device)
        ctx.save_for_backward(rows, tape)
        ctx.set_materialize_grads(False)                       # (an output nobody differentiates arrives as None: NULL = zeros)
        return obs, kin_k

    @staticmethod
    @once_differentiable
    def backward(ctx, g_obs, g_kin):
        core, K = ctx.core, ctx.K
        rows, tape = ctx.saved_tensors
        dev, N = core.device, core.N
        g_kin = _cot(g_kin, core.kin_store)
        g_rows = torch.empty((K, N, rows.shape[-1]), dtype=torch.float32, device=dev)
        with_gains = ctx.with_gains and ctx.needs_input_grad[7]
        g_table = torch.zeros((12, core.ld), dtype=torch.float32, device=dev) if with_gains else None     # (the kernel writes drones 0 .. N-1)
        sweep_ctbr(core, ctx.ctbr, ctx.mode, K, rows, ctx.r_stride, tape, _cot(g_obs), g_kin, g_rows, g_table, ctx.plant)
        g_gains = None
        if with_gains:         # the forward's gains are shared: the sum over drones, in float64 (N terms), in the caller's shape and place
            shape, dtype, device = ctx.gains_like
            g_gains = g_table[:, :N].sum(dim=1, dtype=torch.float64).reshape(4, 3).to(device=device, dtype=dtype).reshape(shape)
        return None, None, g_kin, _action_grad(g_rows, ctx.r_stride, rows), None, None, None, g_gains


def rollout_diff_ctbr(core, ctrl, rows, kin0=None, num_steps: int = None, mode: str = "cmd", gains=None):
    """`SimCore.rollout_diff_ctbr`: K control steps on thrust and body-rate commands in one launch (`SimCore.rollout_ctbr`'s flight),
    differentiable with respect to `rows`, `kin0` and `gains`.

    `ctrl`: a `control.VectorCTBR` with one controller per drone.  `rows`: in `mode="cmd"` commands `[K, N, 4]`, or -- with
    `num_steps=K` -- ONE block `[N, 4]` held for all K steps (its gradient is the sum over the steps); in `mode="pos"` targets
    `[K, N, 12]` / `[N, 12]` (pos | rpy | vel | rpy rates; rows of 3 floats are positions), whose rpy and rate slots -- ignored by the
    forward -- receive exact zeros.  `kin0`: None (the core's own state) or a `[13 * ld]` tensor in the plane layout (`pack_kin`),
    copied into the state first.  Returns fresh tensors `(obs12 [K,N,12], kin_K [13*ld])`, both carrying gradients; `kin_K` of one
    call as `kin0` of the next chains the graph.  `gains`: None (the controller's own: constants, no gain gradient) or a `[4, 3]`
    tensor, rows `CTBR_GAIN_FIELDS` = k_p, k_d, k_rates, k_rate; it REPLACES the controller's gains for this call (`ctrl` keeps its
    own) and -- when it requires grad -- receives the gradient summed over drones.  Reading its 12 floats to the host is a
    SYNCHRONISATION when it lives on the device.  Single-drone aviaries, no task, the two raw RPM action types, no add-on physics or
    drag, no auto-reset, with or without a plant table (a constant): `GpdError` otherwise."""
    if mode not in _native.CTBR_MODES:
        raise ValueError(f"rollout_diff_ctbr: mode must be 'cmd' or 'pos', got {mode!r}")
    if core.host_visible:
        raise ValueError("rollout_diff_ctbr: a host-visible core steps one aviary at a time (CtrlAviary.step takes RPMs)")
    if core.act_ring is not None:
        raise ValueError("rollout_diff_ctbr: this core keeps an action history, which the fused rollout would not advance")
    if getattr(ctrl, "n", None) != core.N or ctrl.device != core.device or not hasattr(ctrl, "thrust_max"):
        raise ValueError(f"rollout_diff_ctbr needs a VectorCTBR of {core.N} controllers on {core.device}")
    if gains is not None and (not isinstance(gains, torch.Tensor) or gains.numel() != 12):
        raise ValueError("gains must be a tensor of 4 x 3 gains (rows: k_p, k_d, k_rates, k_rate)")
    t = rows if isinstance(rows, torch.Tensor) else torch.as_tensor(rows, dtype=torch.float32)
    t = t.to(device=core.device, dtype=torch.float32)
    W = 4 if mode == "cmd" else 12
    if mode == "pos" and t.dim() >= 2 and t.shape[-1] == 3:
        t = torch.cat([t, torch.zeros(t.shape[:-1] + (9,), dtype=torch.float32, device=core.device)], dim=-1)
    if t.dim() == 3 and num_steps is None:
        num_steps = t.shape[0]
    if num_steps is None or int(num_steps) < 1:
        raise ValueError("num_steps must be >= 1 (it may be left out only with one block of rows per step)")
    K = int(num_steps)
    if tuple(t.shape) == (core.N, W):
        r_stride = 0
    elif tuple(t.shape) == (K, core.N, W):
        r_stride = core.N * W
    else:
        raise ValueError(f"rows must be [{core.N}, {W}] or [{K}, {core.N}, {W}]" + (" (or rows of 3: positions)" if mode == "pos" else "")
                         + f" in mode {mode!r}, got {tuple(t.shape)}")
    tape_floats_ctbr(core, K)                                  # (the configuration check, with the library's message, before anything else)
    if core._state.dw_force:
        raise _native.GpdError("rollout_diff_ctbr: downwash computed outside the kernel (state.dw_force) is not differentiable")
    kin0 = _state0(core, kin0, core.kin_store, "kin0", "the plane layout: pack_kin")
    return RolloutDiffCtbr.apply(core, ctrl.struct(), kin0, t.contiguous(), K, r_stride, mode, gains)
