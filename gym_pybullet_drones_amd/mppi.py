"""Sampling-based model-predictive control on the device: the binding of `gpd_mppi` (include/gpd.h) and of
`gpd_mppi_ctbr`, the same planner over thrust and body-rate commands (section 3.19), and of `gpd_mppi_peers`, either of them with the
other drones' published paths in the cost (section 3.20), and of `gpd_mppi_plant`, either of them on the aviary's own model (section 3.21).

Per drone, M perturbed action sequences around a nominal one are rolled H env steps through the in-register physics, scored, and the
nominal is replaced by their cost-weighted average (MPPI, Williams et al.): one launch per plan, no trajectory in memory.  The
reference has no planner; its examples steer by hand-written DSLPID set-points.

The planning model is a single drone without episode ends, and `MPPI` / `CTBRMPPI` offer two of them.  `model="nominal"` (the default)
is the nominal airframe under the flag-less DYN integrator, whatever the environment flies: no drag, ground effect, ground plane or
damping, and no plant table -- a plan under a simpler model, as in any MPC.  `model="aviary"` is the core's own model: its
`physics_flags` (ground effect, drag, the ground plane, damping) and, per drone, whatever plant table the core holds at each launch
(`SimCore.set_plant`, `VectorAviary(randomize=...)`), or the planner's own belief about the airframes (`plant=`, `set_plant`), which is
where an identified airframe (examples/sysid.py) goes.  Downwash is in neither model (it needs mates), and `SwarmMPPI` plans on the
nominal model only.
"""
import ctypes
import dataclasses
import math

import torch

from . import _native
from . import neighbors as _nb
from . import obstacles as _ob
from .utils.enums import PHYS_DW

MODELS = ("nominal", "aviary")

ACT_RPM, ACT_VEL = 0, 2
ACT_RAW_RPM, ACT_DIRECT_RPM = 5, 6        # what `CTBRMPPI`'s core flies (the rate loop's output is RPMs)
#: the default bounds of a sample's action: [-1, 1]^4 for RPM; a direction in [-1, 1]^3 and a speed fraction in [0, 1] for VEL
DEFAULT_BOUNDS = {ACT_RPM: ((-1.0,) * 4, (1.0,) * 4), ACT_VEL: ((-1.0, -1.0, -1.0, 0.0), (1.0, 1.0, 1.0, 1.0))}


@dataclasses.dataclass
class MPPICost:
    """The running cost of the state after each step (include/gpd.h):
    `w_pos |p - goal|^2` (times `w_term` on the last step) `+ w_vel |v|^2 + w_tilt (1 - R22) + w_rate |omega_body|^2
    + w_obs max(0, obst_margin - (d - collision_radius))^2`; `collision_radius` None: the airframe's `COLLISION_R`."""
    w_pos: float = 1.0
    w_vel: float = 0.05
    w_tilt: float = 0.5
    w_rate: float = 0.01
    w_term: float = 5.0
    w_obs: float = 100.0
    obst_margin: float = 0.3
    collision_radius: float = None


class _Planner:
    """What `MPPI` and `CTBRMPPI` share: the sampler's struct, the model's configuration, the tensors, and `nominal` / `plan` /
    `advance` / `reset`.  A subclass checks its core, then calls `_bind` with its default bounds; it names its entry (`_ENTRY`), the
    arguments in front of `GpdState` (`_lead`) and its hover action (`_hover`)."""
    _ENTRY = None
    model = "nominal"
    #: the planner's own belief about the airframes (`plant=` / `set_plant`): [9, ld] scales and the [19, ld] derived rows; None: the
    #: core's table, whatever it is at each launch
    plant_scales = None
    plant_rows = None

    def _bind(self, core, horizon, samples, sigma, lam, cost, seed, field, lo, hi, act_lo, act_hi, model="nominal", plant=None):
        self.core, self.device, self.N = core, core.device, core.N
        if model not in MODELS:
            raise ValueError(f"model must be one of {MODELS}")
        if plant is not None and model != "aviary":
            raise ValueError('plant= is the belief of model="aviary"; the nominal model flies the nominal airframe')
        if model == "aviary" and ((core.physics_flags & PHYS_DW) or core._state.dw_force):
            raise ValueError('model="aviary" has no downwash (it needs mates): the core has GPD_PHYS_DW or computes it outside the kernel')
        self.model = model
        self.H, self.M = int(horizon), int(samples)
        if self.H < 1 or self.M % 64 != 0 or not 64 <= self.M <= 1024:
            raise ValueError("horizon must be >= 1 and samples a multiple of 64 in 64..1024")
        if not (lam > 0.0 and math.isfinite(lam)):
            raise ValueError("lam must be positive and finite")
        cost = MPPICost() if cost is None else cost
        lo, hi = (lo if act_lo is None else tuple(act_lo)), (hi if act_hi is None else tuple(act_hi))
        sigma = (float(sigma),) * 4 if isinstance(sigma, (int, float)) else tuple(float(s) for s in sigma)
        if len(sigma) != 4 or len(lo) != 4 or len(hi) != 4:
            raise ValueError("sigma, act_lo and act_hi have 4 components")
        radius = core.P.COLLISION_R if cost.collision_radius is None else cost.collision_radius
        seed = int(seed)
        F4 = ctypes.c_float * 4
        self._q = _native.GpdMppi(horizon=self.H, samples=self.M, sigma=F4(*sigma), act_lo=F4(*lo), act_hi=F4(*hi), lam=lam, w_pos=cost.w_pos,
                                  w_vel=cost.w_vel, w_tilt=cost.w_tilt, w_rate=cost.w_rate, w_term=cost.w_term, w_obs=cost.w_obs,
                                  obst_margin=cost.obst_margin, collision_radius=radius,
                                  seed=(ctypes.c_uint32 * 2)(seed & 0xFFFFFFFF, (seed >> 32) & 0xFFFFFFFF), iteration=0)
        # the model's configuration: the core's rates and action type, nothing else of it
        c = core._cfg
        self._cfg = _native.GpdStepCfg(num_envs=core.E, drones_per_env=1, act_type=core.act_code, substeps=core.S,
                                       physics_flags=core.physics_flags if model == "aviary" else 0,
                                       pyb_dt=c.pyb_dt, ctrl_dt=c.ctrl_dt, inv_ctrl_dt=c.inv_ctrl_dt, lanes_per_wave=c.lanes_per_wave,
                                       task=0, auto_reset=0)
        if isinstance(field, _ob.ObstacleField):
            field = _ob.FieldQuery(field, self.device, self.N, 1, radius)
        # (gpd_obstacles names the shared list by a pitch of 1, gpd_mppi by 0; one aviary's own list at pitch 1 is the same bytes)
        self._obst = (None, 0, 0) if field is None else (field.obst, field.n_obst, 0 if field.obst_ld == 1 else field.obst_ld)
        f32 = dict(dtype=torch.float32, device=self.device)
        self._u = [torch.zeros((self.H, self.N, 4), **f32), torch.zeros((self.H, self.N, 4), **f32)]
        self._goal = torch.zeros((self.N, 4), **f32)
        self.costs, self.stats = torch.zeros((self.N, self.M), **f32), torch.zeros((self.N, 4), **f32)
        self.iteration = 0
        if plant is not None:
            self.set_plant(plant)
        self.reset()

    # (what `SimCore._plant_input` reads of its core: the belief is parsed and completed exactly as the core's own table is)
    E = property(lambda self: self.N)
    D = 1

    def plant_view(self) -> torch.Tensor:
        """[9, N, 1] VIEW of the belief's scale table (None without one)."""
        return None if self.plant_scales is None else self.plant_scales[:, :self.N].view(-1, self.N, 1)

    def set_plant(self, scales, mask=None):
        """Set the planner's OWN BELIEF about the airframes (`model="aviary"` only): anything `SimCore.set_plant` accepts -- a tensor
        `[9, N]` / `[9, N, 1]` of scale factors or a dict {field: tensor / scalar}, fields left out keeping the belief's current values
        (1.0 on first use); `mask` (bool/uint8 [N]): only those drones change.  The rows are derived through `gpd_plant_derive`, used
        in place of the core's table from the next launch on, and never written to the core.  One host sync (the validation)."""
        if self.model != "aviary":
            raise ValueError('set_plant: the belief belongs to model="aviary"')
        c = self.core
        full = type(c)._plant_input(self, scales)
        if bool((~(torch.isfinite(full) & (full > 0))).any()):
            raise ValueError("set_plant: every scale must be finite and > 0")
        first = self.plant_scales is None
        if first:
            self.plant_scales = torch.ones((len(_native.SCALE_FIELDS), c.ld), dtype=torch.float32, device=self.device)
            self.plant_rows = torch.empty((_native.PLANT_ROWS, c.ld), dtype=torch.float32, device=self.device)
        view = self.plant_view()
        if mask is not None:
            mask = mask.to(device=self.device, dtype=torch.uint8).contiguous()
            torch.where(mask.view(1, self.N, 1).bool(), full, view, out=view)
        else:
            view.copy_(full)
        _native.call("gpd_plant_derive", self.device, c._stream(), c._params, self.plant_scales, None if first else mask, self.N, 1, c.ld,
                     self.plant_rows)

    def _ctbr(self):
        """the model's `GpdCtbr` (None: RPM / VEL actions), as `gpd_mppi_plant` takes it"""
        return None

    @property
    def nominal(self) -> torch.Tensor:
        """the nominal action sequence `[H, N, 4]` (the tensor the next plan starts from)"""
        return self._u[0]

    def _lead(self) -> tuple:
        """the entry's arguments in front of `GpdState`"""
        return (self.core._params,)

    def _hover(self) -> tuple:
        raise NotImplementedError

    def reset(self, rows=None, value=None):
        """Set the nominal of the drones `rows` (index or mask tensor; None: all) to `value` (4 numbers or `[.., 4]`; None: hover --
        zeros for RPM, a zero speed along +x for VEL, which commands a stop, the thrust g without rates for CTBR)."""
        if value is None:
            value = self._hover()
        v = torch.as_tensor(value, dtype=torch.float32, device=self.device)
        if rows is None:
            self._u[0][:] = v
        else:
            self._u[0][:, rows] = v

    def _launch(self, goal, goal_stride):
        self._q.iteration = self.iteration & 0xFFFFFFFF
        obst, n_obst, ld = self._obst
        c = self.core
        if self.model == "aviary":         # the belief, else the core's table AS IT IS NOW (None: the nominal airframe)
            rows = self.plant_rows if self.plant_rows is not None else c.plant_rows
            _native.call("gpd_mppi_plant", self.device, c._stream(), c._params, self._ctbr(), c._state, self._cfg, self._q, rows, self._u[0],
                         self.N * 4, goal, goal_stride, obst, n_obst, ld, self._u[1], self.costs, self.stats)
        else:
            _native.call(self._ENTRY, self.device, c._stream(), *self._lead(), c._state, self._cfg, self._q, self._u[0], self.N * 4, goal,
                         goal_stride, obst, n_obst, ld, self._u[1], self.costs, self.stats)
        self._u.reverse()
        self.iteration += 1

    def plan(self, goal, iterations: int = 1) -> torch.Tensor:
        """Run `iterations` updates of the nominal from the core's CURRENT state towards `goal` -- `[N, 3]` (one goal per drone for the
        whole horizon), `[3]` (the same for all), or a float32 device tensor `[H, N, 4]` of xyz-padded goals per step, used as it is --
        and return the first action of the nominal, `[N, 4]`.  The state is not touched; no host synchronisation."""
        g = goal if isinstance(goal, torch.Tensor) else torch.as_tensor(goal, dtype=torch.float32)
        if g.ndim == 3:
            if tuple(g.shape) != (self.H, self.N, 4) or g.dtype != torch.float32 or g.device != self.device or not g.is_contiguous():
                raise ValueError(f"a goal per step is a contiguous float32 device tensor [{self.H}, {self.N}, 4]")
            buf, stride = g, self.N * 4
        else:
            self._goal[:, :3] = g.to(self.device, torch.float32)
            buf, stride = self._goal, 0
        for _ in range(int(iterations)):
            self._launch(buf, stride)
        return self._u[0][0]

    def advance(self):
        """The warm start of the next plan: shift the nominal one step, repeating its last row."""
        u, v = self._u
        if self.H > 1:
            v[:-1] = u[1:]
        v[-1] = u[-1]
        self._u.reverse()


class MPPI(_Planner):
    """A planner bound to a `SimCore` of single drones with RPM or VEL actions: the nominal sequence `[H, N, 4]`, the samples' `costs`
    `[N, M]` and `stats` `[N, 4]` (min cost, weighted mean cost, effective sample size, finite samples) are tensors allocated once;
    every launch goes to the core's stream.  `field`: an `obstacles.ObstacleField` (or the `FieldQuery` an aviary built from one).
    `model`: "nominal" (`gpd_mppi`: the nominal airframe, no physics flags) or "aviary" (`gpd_mppi_plant`: the core's physics flags and
    its plant table at each launch, or the belief `plant` -- anything `SimCore.set_plant` accepts; `set_plant` updates it)."""
    _ENTRY = "gpd_mppi"

    def __init__(self, core, horizon: int, samples: int, sigma, lam: float, cost: MPPICost = None, seed: int = 0, field=None,
                 act_lo=None, act_hi=None, model: str = "nominal", plant=None):
        if core.D != 1:
            raise ValueError("MPPI plans for aviaries of one drone (drones_per_env must be 1)")
        if core.act_code not in DEFAULT_BOUNDS:
            raise ValueError("MPPI plans over RPM or VEL actions (ActionType.RPM / ActionType.VEL)")
        self._bind(core, horizon, samples, sigma, lam, cost, seed, field, *DEFAULT_BOUNDS[core.act_code], act_lo, act_hi, model, plant)

    def _hover(self) -> tuple:
        return (0.0, 0.0, 0.0, 0.0) if self.core.act_code == ACT_RPM else (1.0, 0.0, 0.0, 0.0)


class CTBRMPPI(_Planner):
    """`MPPI` over thrust and body-rate commands (`gpd_mppi_ctbr`): a sample's action is a command `(thrust
    [m/s^2], body rates x, y, z [rad/s])` held over the control step, and the model runs `ctrl`'s body-rate loop inside every physics
    sub-step, exactly as `SimCore.rollout_ctbr(ctrl, cmd, K, mode="cmd")` flies it.  `core`: aviaries of one drone with RAW_RPM or
    DIRECT_RPM actions (`VectorCtrlAviary`), what `rollout_ctbr` requires; `ctrl`: a `control.VectorCTBR` of `core.N` controllers on
    the core's device.  The default bounds are the controller's clips, `(0, -rate_max x 3) .. (thrust_max, +rate_max x 3)`; wider ones
    are legal, the rate loop clips.  The default nominal is the hover command `(g, 0, 0, 0)` with the controller's `g`.  `plan()`
    returns `[N, 4]` commands for `rollout_ctbr(ctrl, cmd, 1, mode="cmd")`.  `model`, `plant`: as for `MPPI` ("aviary": the model is
    `rollout_ctbr`'s on the core's physics flags and plant table; the rate loop stays on the nominal M and J)."""
    _ENTRY = "gpd_mppi_ctbr"

    def __init__(self, core, ctrl, horizon: int, samples: int, sigma, lam: float, cost: MPPICost = None, seed: int = 0, field=None,
                 act_lo=None, act_hi=None, model: str = "nominal", plant=None):
        if core.D != 1:
            raise ValueError("CTBRMPPI plans for aviaries of one drone (drones_per_env must be 1)")
        if core.act_code not in (ACT_RAW_RPM, ACT_DIRECT_RPM):
            raise ValueError("CTBRMPPI needs a core with RAW_RPM or DIRECT_RPM actions (the rate loop's output is RPMs), as rollout_ctbr")
        if getattr(ctrl, "n", None) != core.N or ctrl.device != core.device or not hasattr(ctrl, "thrust_max"):
            raise ValueError(f"CTBRMPPI needs a VectorCTBR of {core.N} controllers on {core.device}")
        self.ctrl = ctrl
        r = ctrl.rate_max
        self._bind(core, horizon, samples, sigma, lam, cost, seed, field, (0.0, -r, -r, -r), (ctrl.thrust_max, r, r, r), act_lo, act_hi, model, plant)

    def _lead(self) -> tuple:
        return (self.core._params, self.ctrl.struct())

    def _ctbr(self):
        return self.ctrl.struct()

    def _hover(self) -> tuple:
        return (float(self.ctrl.struct().g), 0.0, 0.0, 0.0)


class SwarmMPPI(_Planner):
    """`MPPI` (`ctrl=None`: a core of single drones with RPM or VEL actions) or `CTBRMPPI` (`ctrl`: a `control.VectorCTBR`; a core with
    RAW_RPM or DIRECT_RPM actions) for drones that SHARE ONE AIRSPACE (`gpd_mppi_peers`): the N single-drone
    aviaries of `core` are taken to fly in the same world, and the running cost gets `w_peer * sum_j max(0, peer_dist - |p - p_j(h)|)^2`
    over the drone's `k` nearest peers within `radius`, p_j(h) where peer j last PUBLISHED it would be after step h.  Every launch plans
    all drones against table A of published paths `[H, N + intruders, 4]` and publishes the paths of the new nominals into table B,
    then the tables swap: every drone answers its peers' previous paths (a Jacobi iteration), all in one launch, decentralised.

    `peer_dist` None: `2 * COLLISION_R + cost.obst_margin` (two hulls and the margin the obstacles get).  `radius` None:
    `peer_dist + 2 * SPEED_LIMIT * horizon * ctrl_dt` -- two drones that fly at each other at the speed limit for the whole horizon
    close that much; a peer beyond it cannot come within `peer_dist` inside the horizon.  `intruders`: rows N .. N + intruders - 1 of
    the tables are other moving bodies whose paths the caller gives to `plan()`; every drone counts every one of them
    (`k + intruders <= 32`).  `box` (x0, y0, x1, y1): the neighbour search's grid; None: the bounds of the current positions padded by
    `radius`, recomputed by `reset()` (it changes the search's speed, never its result).  `SwarmAviary` has no binding: its core runs
    one sub-step per control step, and a multi-rank world numbers peers across ranks."""
    _ENTRY = "gpd_mppi_peers"

    def __init__(self, core, horizon: int, samples: int, sigma, lam: float, cost: MPPICost = None, seed: int = 0, field=None, ctrl=None,
                 k: int = 8, radius: float = None, w_peer: float = 100.0, peer_dist: float = None, intruders: int = 0, box=None,
                 act_lo=None, act_hi=None):
        if core.D != 1:
            raise ValueError("SwarmMPPI plans for aviaries of one drone (drones_per_env must be 1)")
        if ctrl is None:
            if core.act_code not in DEFAULT_BOUNDS:
                raise ValueError("SwarmMPPI without ctrl plans over RPM or VEL actions (ActionType.RPM / ActionType.VEL)")
            lo, hi = DEFAULT_BOUNDS[core.act_code]
        else:
            if core.act_code not in (ACT_RAW_RPM, ACT_DIRECT_RPM):
                raise ValueError("SwarmMPPI with ctrl needs a core with RAW_RPM or DIRECT_RPM actions (the rate loop's output is RPMs), as rollout_ctbr")
            if getattr(ctrl, "n", None) != core.N or ctrl.device != core.device or not hasattr(ctrl, "thrust_max"):
                raise ValueError(f"SwarmMPPI needs a VectorCTBR of {core.N} controllers on {core.device}")
            r = ctrl.rate_max
            lo, hi = (0.0, -r, -r, -r), (ctrl.thrust_max, r, r, r)
        self.ctrl, self.intruders = ctrl, int(intruders)
        cost = MPPICost() if cost is None else cost
        peer_dist = 2.0 * core.P.COLLISION_R + cost.obst_margin if peer_dist is None else float(peer_dist)
        w_peer = float(w_peer)
        if not (w_peer >= 0.0 and math.isfinite(w_peer) and peer_dist >= 0.0 and math.isfinite(peer_dist)):
            raise ValueError("w_peer and peer_dist must be non-negative and finite")
        if self.intruders < 0 or int(k) + self.intruders > _nb.MAX_K:
            raise ValueError(f"intruders must be >= 0 and k + intruders <= {_nb.MAX_K}")
        if int(horizon) < 1:
            raise ValueError("horizon must be >= 1 and samples a multiple of 64 in 64..1024")
        radius = peer_dist + 2.0 * core.P.SPEED_LIMIT * int(horizon) * core._cfg.ctrl_dt if radius is None else radius
        self.radius, self.k = _nb.check_args(radius, k)
        self.peer_dist, self.w_peer, self._box = peer_dist, w_peer, None if box is None else tuple(float(v) for v in box)
        self._paths = None
        self._bind(core, horizon, samples, sigma, lam, cost, seed, field, lo, hi, act_lo, act_hi)
        # the nominals and the tables share ONE row stride, N + intruders rows: path_out has the layout and stride of u_out
        rows, f32 = self.N + self.intruders, dict(dtype=torch.float32, device=self.device)
        self._rows = rows
        if self.intruders:
            self._u = [torch.zeros((self.H, rows, 4), **f32)[:, :self.N] for _ in range(2)]
        self._paths = [torch.full((self.H, rows, 4), float("nan"), **f32) for _ in range(2)]
        self._idx = torch.full((self.N, self.k + self.intruders), -1, dtype=torch.int32, device=self.device)
        if self.intruders:
            self._idx[:, self.k:] = torch.arange(self.N, rows, dtype=torch.int32, device=self.device)
        self._r = _native.GpdMppiPeers(idx=self._idx.data_ptr(), pos_step_stride=rows * 4, k=self.k + self.intruders, idx_ld=self.k + self.intruders,
                                       n_rows=rows, w_peer=w_peer, peer_dist=peer_dist)
        self.reset()

    def _hover(self) -> tuple:
        if self.ctrl is not None:
            return (float(self.ctrl.struct().g), 0.0, 0.0, 0.0)
        return (0.0, 0.0, 0.0, 0.0) if self.core.act_code == ACT_RPM else (1.0, 0.0, 0.0, 0.0)

    @property
    def paths(self) -> torch.Tensor:
        """the published paths `[H, N, 4]`: x, y, z after each step of the nominal, and the distance to the nearest counted peer there"""
        return self._paths[0][:, :self.N]

    @property
    def min_separation(self) -> torch.Tensor:
        """`[N]`: the smallest distance to a counted peer's published path along the drone's own published path (+inf: no peer)"""
        return self.paths[..., 3].amin(dim=0)

    def reset(self, rows=None, value=None):
        """`_Planner.reset`, and the published paths are forgotten: the next `plan()` starts from constant-velocity paths.  Without a
        `box` the search's grid is laid over the current positions again (one host synchronisation)."""
        super().reset(rows, value)
        if self._paths is None:             # (the base's own call, before the tables exist)
            return
        self._published = False
        box = self._box
        if box is None:
            p = self.core.kin_P[:self.N, :2]
            lo, hi = p.amin(dim=0).tolist(), p.amax(dim=0).tolist()
            box = (lo[0] - self.radius, lo[1] - self.radius, hi[0] + self.radius, hi[1] + self.radius)
        self.search = _nb.WorldSearch(self.device, self.N, 0, self.N, self.radius, self.k, box, rel=False)

    def _launch(self, goal, goal_stride):
        self._q.iteration = self.iteration & 0xFFFFFFFF
        obst, n_obst, ld = self._obst
        c, r = self.core, self._r
        r.pos, r.path_out = self._paths[0].data_ptr(), self._paths[1].data_ptr()
        _native.call(self._ENTRY, self.device, c._stream(), c._params, None if self.ctrl is None else self.ctrl.struct(), c._state, self._cfg,
                     self._q, r, self._u[0], self._rows * 4, goal, goal_stride, obst, n_obst, ld, self._u[1], self.costs, self.stats)
        if self.intruders:
            self._paths[1][:, self.N:] = self._paths[0][:, self.N:]
        self._u.reverse()
        self._paths.reverse()
        self.iteration += 1

    def plan(self, goal, iterations: int = 1, intruder_paths=None) -> torch.Tensor:
        """`_Planner.plan` against the peers: the k-nearest lists are refreshed ONCE per call from the current positions; if nothing is
        published yet (or after `reset()`) the table is filled by constant velocity from the current state; then `iterations`
        launches, each reading table A and writing the drones' rows of table B, then swapping.  `intruder_paths` `[H, intruders, 3]`
        (or `[.., 4]`): where the other bodies will be after each step; None: the rows stay what they were (NaN, not counted, until
        given once).  No host synchronisation."""
        c = self.core
        found = self.search(c.kin_P, c._stream())
        self._idx[:, :self.k] = found.idx
        if not self._published:
            steps = torch.arange(1, self.H + 1, dtype=torch.float32, device=self.device)[:, None, None] * self._cfg.ctrl_dt
            self._paths[0][:, :self.N, :3] = c.kin_P[None, :self.N, :3] + steps * c.kin_V[None, :self.N, :3]
            self._paths[0][:, :self.N, 3] = 0.0
            self._published = True
        if intruder_paths is not None:
            t = torch.as_tensor(intruder_paths, dtype=torch.float32, device=self.device)
            self._paths[0][:, self.N:, :t.shape[-1]] = t
        return super().plan(goal, iterations)

    def advance(self):
        """The warm start of the next plan: shift the nominal AND the published paths one step, repeating their last rows."""
        super().advance()
        a, b = self._paths
        if self.H > 1:
            b[:-1] = a[1:]
        b[-1] = a[-1]
        self._paths.reverse()
