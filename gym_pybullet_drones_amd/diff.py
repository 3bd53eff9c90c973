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


class RolloutDiff(torch.autograd.Function):
    """forward: `gpd_rollout_tape` from `kin0` (copied into the core's state first); backward: `gpd_rollout_vjp`, or -- when
    `plant_scales` (the scales `rollout_diff` has just installed with `set_plant`) asks for a gradient -- `gpd_rollout_vjp_plant`
    and `gpd_plant_derive_vjp`"""

    @staticmethod
    def forward(ctx, core, kin0, actions, K, a_stride, plant_scales=None, own_plant=False):
        dev, N, E = core.device, core.N, core.E
        size = tape_floats(core, K)                            # (also the configuration check, before anything is touched)
        if kin0.data_ptr() != core.kin_store.data_ptr():
            core.kin_store.copy_(kin0)
        obs = torch.empty((K, N, 12), dtype=torch.float32, device=dev)
        rew = torch.empty((K, E), dtype=torch.float32, device=dev)
        term = torch.empty((K, E), dtype=torch.bool, device=dev)
        trunc = torch.empty((K, E), dtype=torch.bool, device=dev)
        tape = torch.empty((size,), dtype=torch.float32, device=dev)
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
        g_obs = None if g_obs is None else g_obs.to(torch.float32).contiguous()
        g_rew = None if g_rew is None else g_rew.to(torch.float32).contiguous()
        g_kin = torch.zeros_like(core.kin_store) if g_kin is None else g_kin.to(torch.float32).clone(memory_format=torch.contiguous_format)
        g_act = torch.empty((K, N, core.A), dtype=torch.float32, device=dev)
        with_scales = ctx.scales is not None and ctx.needs_input_grad[5]
        g_rows = torch.empty((_native.PLANT_ROWS, core.ld), dtype=torch.float32, device=dev) if with_scales else None     # (both kernels write drones 0 .. N-1)
        sweep(core, K, actions, ctx.a_stride, tape, g_obs, g_rew, g_kin, g_act, ctx.target, ctx.plant, g_rows)
        g_scales = None
        if with_scales:
            g_table = torch.empty((len(_native.SCALE_FIELDS), core.ld), dtype=torch.float32, device=dev)
            derive_vjp(core, ctx.scales, g_rows, g_table)
            g_scales = g_table[:, :N].reshape(ctx.scales_shape)
        if ctx.a_stride == 0:                                  # a shared action block: its gradient is the sum over the steps
            g_act = g_act.sum(dim=0)
        return None, g_kin, g_act.view(actions.shape), None, None, g_scales, None


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
    if kin0 is None:
        kin0 = core.kin_store.detach()
    else:
        if kin0.numel() != 13 * core.ld:
            raise ValueError(f"kin0 has {kin0.numel()} elements, expected 13 x ld = {13 * core.ld} (the plane layout: pack_kin)")
        kin0 = kin0.to(device=core.device, dtype=torch.float32).reshape(-1).contiguous()
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
