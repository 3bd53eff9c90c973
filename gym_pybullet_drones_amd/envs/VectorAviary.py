"""Batched aviaries: E independent Hover / MultiHover / control aviaries advanced by ONE kernel launch.

New relative to the reference, which vectorises only through SB3's `make_vec_env(..., n_envs=1)`
(`examples/learn.py:54-58`).  The per-aviary semantics are exactly those of `HoverAviary` /
`MultiHoverAviary` / `CtrlAviary`; on top of that the batch follows the SB3 `DummyVecEnv`
convention: an aviary that terminates or is truncated is reset inside the same `step()` and the
observation returned for it is the first one of the new episode (the last one of the finished
episode is available as `info["terminal_observation"]` when `keep_terminal_obs=True`).  As in the
reference, a reset neither clears the action history nor the embedded PID state
(SURVEY.md App. B.2/B.3).

Everything stays on the GPU: actions come in and observations / rewards / flags go out as torch
tensors on the aviary's device, nothing synchronises with the host.
"""
import math

import numpy as np
import torch

from .. import _native, engine, mppi as _mppi, neighbors as _nb, obstacles as _ob
from ..params import DroneParams
from ..utils.enums import ACT_RAW_RPM, ActionType, DroneModel, ObservationType, Physics

_TASKS = {"none": engine.TASK_NONE, "hover": engine.TASK_HOVER, "multihover": engine.TASK_MULTIHOVER}


class VectorAviary:
    """E aviaries x D drones.  Observations `(E, D, 12)` (or `(E, D, 12 + H*A)` with `full_obs`)."""

    def __init__(self,
                 num_envs: int,
                 num_drones: int = 1,
                 drone_model: DroneModel = DroneModel.CF2X,
                 initial_xyzs=None,
                 initial_rpys=None,
                 physics: Physics = Physics.DYN,
                 pyb_freq: int = 240,
                 ctrl_freq: int = 30,
                 obs: ObservationType = ObservationType.KIN,
                 act=ActionType.RPM,
                 task: str = "hover",
                 target_pos=None,
                 episode_len_sec: float = 8,
                 auto_reset: bool = True,
                 full_obs: bool = False,
                 keep_terminal_obs: bool = False,
                 track_rpm: bool = False,
                 pyb_like: bool = None,
                 nan_guard: bool = False,
                 randomize: dict = None,
                 neighbourhood_radius: float = np.inf,
                 device=None):
        """`randomize`: domain randomisation of the plant, {field: r} with a field of `_native.SCALE_FIELDS` (mass, ixx, iyy, izz,
        kf, km, drag_xy, drag_z, gnd_eff) and 0 <= r < 1 -- every drone's scale of that field is drawn from U(1 - r, 1 + r) at
        construction, for the aviaries `reset()` resets (seeded by its `seed`), and for the aviaries that end and auto-reset in
        `step()`.  See `set_physical_params` for what the scales change and what stays nominal."""
        if obs != ObservationType.KIN:
            raise NotImplementedError("only ObservationType.KIN is on the MI355X hot path")
        self.randomize = self._check_randomize(randomize)      # (before any device work)
        self.NUM_ENVS, self.NUM_DRONES = int(num_envs), int(num_drones)
        self.NEIGHBOURHOOD_RADIUS = neighbourhood_radius         # (envs/BaseAviary.py:124; used by neighbors() / adjacency())
        self.DRONE_MODEL, self.PHYSICS = drone_model, physics
        self.PYB_FREQ, self.CTRL_FREQ = pyb_freq, ctrl_freq
        self.PYB_STEPS_PER_CTRL = pyb_freq // ctrl_freq
        self.CTRL_TIMESTEP, self.PYB_TIMESTEP = 1. / ctrl_freq, 1. / pyb_freq
        self.EPISODE_LEN_SEC = episode_len_sec
        self.ACT_TYPE = act
        act_code = ACT_RAW_RPM if act == "raw_rpm" else act.code
        P = DroneParams(drone_model)
        self.HOVER_RPM, self.MAX_RPM = P.HOVER_RPM, P.MAX_RPM
        if initial_xyzs is None:
            initial_xyzs = P.default_init_xyzs(self.NUM_DRONES)
        init = np.asarray(initial_xyzs, dtype=np.float64)
        if target_pos is None:
            if task == "hover":
                target_pos = np.broadcast_to(np.array([0., 0., 1.]), (self.NUM_DRONES, 3)).copy()
            elif task == "multihover":
                target_pos = init + np.array([[0, 0, 1 / (i + 1)] for i in range(self.NUM_DRONES)])
        xy = 1.5 if task == "hover" else 2.0
        self.core = engine.SimCore(drone_model=drone_model, num_envs=num_envs, drones_per_env=num_drones,
                                   physics=physics, pyb_freq=pyb_freq, ctrl_freq=ctrl_freq, act_code=act_code,
                                   task=_TASKS[task], initial_xyzs=init, initial_rpys=initial_rpys,
                                   target_pos=target_pos, episode_len_sec=episode_len_sec, xy_bound=xy,
                                   auto_reset=auto_reset, track_rpm=track_rpm, keep_terminal_obs=keep_terminal_obs,
                                   device=device, pyb_like=pyb_like, nan_guard=nan_guard)
        self.device = self.core.device
        self.ACT_DIM = self.core.A
        self.INIT_XYZS, self.INIT_RPYS, self.TARGET_POS = self.core.INIT_XYZS, self.core.INIT_RPYS, self.core.TARGET_POS
        # full_obs: False -> (E, D, 12) rows only, no action history kept;
        #           True  -> the reference's (E, D, 12 + H*A) rows, materialised after every step (one gather kernel);
        #           "lazy" -> the action ring is kept (pushed inside the step kernel, +2 x 16 B per drone and step) and
        #                     step() returns the (E, D, 12) rows; `history()` is a zero-copy strided view of the ring,
        #                     `full_rows()` materialises the reference's rows when a consumer wants them
        if full_obs not in (False, True, "lazy"):
            raise ValueError("full_obs must be False, True or 'lazy'")
        self.lazy_history = full_obs == "lazy"
        self.full_obs = full_obs is True
        self.ACTION_BUFFER_SIZE = int(ctrl_freq // 2)
        self.OBS_DIM = 12 + (self.ACTION_BUFFER_SIZE * self.ACT_DIM if self.full_obs else 0)
        if full_obs:
            self.core.enable_history(self.ACTION_BUFFER_SIZE)
        if self.randomize:
            self._rng = torch.Generator(device=self.device)
            self._rng.seed()
            self._resample(None)

    # ---- gymnasium-VectorEnv-like surface ----------------------------------------------------
    @property
    def num_envs(self):
        return self.NUM_ENVS

    def _obs(self):
        E, D = self.NUM_ENVS, self.NUM_DRONES
        if not self.full_obs:
            return self.core.obs12.view(E, D, 12)
        return self.core.obs_full.view(E, D, self.OBS_DIM)

    def history(self) -> torch.Tensor:
        """(E, D, H, A) zero-copy strided VIEW of the action ring: the last H actions of every drone, oldest first
        (the tail the reference appends to the observation row, BaseRLAviary.py:317-318).  Valid until the next step."""
        H = self.ACTION_BUFFER_SIZE
        return self.core.history_view().unflatten(0, (self.NUM_ENVS, self.NUM_DRONES))

    def action_history(self) -> torch.Tensor:
        """(E*D, H, A) copy of the last H actions, oldest first."""
        return self.core.history_view().contiguous()

    def full_rows(self) -> torch.Tensor:
        """(E, D, 12 + H*A): the reference's observation rows for the current state, materialised now."""
        return self.core.history_rows().view(self.NUM_ENVS, self.NUM_DRONES, -1)

    def reset(self, seed=None, options=None, mask=None):
        """Reset all aviaries (or those selected by the boolean/uint8 tensor `mask` [E]).  As in the reference the
        action history (and the embedded PID state) survives a reset."""
        if self.randomize:     # the reset aviaries fly new airframes
            if seed is not None:
                self._rng.manual_seed(int(seed))
            self._resample(mask)
        self.core.reset(mask=mask)
        if self.full_obs:      # rows of the reset poses with the unchanged history tail (ring not advanced)
            self.core.history_rows()
        return self._obs(), {}

    def step(self, action: torch.Tensor):
        """action: float32 tensor (E, D, A) on `self.device` -> (obs, reward[E], terminated[E], truncated[E], info)."""
        _, reward, terminated, truncated = self.core.step(action)      # (pushes the action into the ring, if there is one)
        if self.randomize and self.core.auto_reset:          # the aviaries that ended were reset by the step: new airframes
            self._resample(terminated | truncated)
        if self.full_obs:
            self.core.history_rows()                         # row assembly: one more launch
        info = {}
        if self.core.term_obs12 is not None:
            info["terminal_observation"] = self.core.term_obs12.view(self.NUM_ENVS, self.NUM_DRONES, 12)
        return self._obs(), reward, terminated, truncated, info

    def rollout(self, actions: torch.Tensor):
        """K env steps in ONE launch (`gpd_rollout`): actions (K, E, D, A) known up front (open-loop sequences,
        DSLPID waypoint lists).  Returns (obs (K,E,D,OBS_DIM), reward (K,E), terminated (K,E), truncated (K,E))."""
        K = actions.shape[0]
        # (lazy history: the rollout kernel pushes the actions into the ring itself when it has a variant for the shape)
        obs, reward, terminated, truncated = self.core.rollout(actions, push_history=bool(self.lazy_history) and not self.full_obs)
        if self.randomize and self.core.auto_reset:
            # an aviary that auto-resets INSIDE the launch keeps its airframe until the launch ends (the kernel has no random numbers);
            # the aviaries that ended at any of the K steps fly new airframes from the next call on
            self._resample((terminated | truncated).any(dim=0))
        if self.full_obs:
            obs = self.core.full_obs(actions, obs12=obs, num_steps=K)
            if self.core.obs_full is None:
                self.core.history_rows()
            self.core.obs_full.copy_(obs[K - 1])
        elif self.lazy_history and not self.core.pushed_history:
            self.core.full_obs(actions, num_steps=K, want_rows=False)      # ring update only
        return obs.view(K, self.NUM_ENVS, self.NUM_DRONES, -1), reward, terminated, truncated

    def rollout_diff(self, actions: torch.Tensor, kin0: torch.Tensor = None, plant_scales=None):
        """The differentiable rollout (`SimCore.rollout_diff`): actions (K, E, 1, A) -> (obs12 (K,E,1,12), reward (K,E), kin_K [13*ld],
        terminated (K,E), truncated (K,E)); obs12, reward and kin_K carry gradients with respect to `actions` and `kin0` (the plane
        layout of the kinematic state, `diff.pack_kin`; None: the current state).  The kinematic rows only: the action history is
        neither pushed nor differentiated.  `plant_scales` ([9, E] / [9, E, 1], or anything else `set_plant` accepts) replaces the
        plant table first, as `set_plant` does, and -- a float tensor that requires grad -- receives its gradient too."""
        obs, reward, kin_k, terminated, truncated = self.core.rollout_diff(actions, kin0, plant_scales=plant_scales)
        return obs.view(-1, self.NUM_ENVS, self.NUM_DRONES, 12), reward, kin_k, terminated, truncated

    def rollout_diff_pid(self, actions: torch.Tensor, kin0: torch.Tensor = None, pid0: torch.Tensor = None, num_steps: int = None,
                         pid_gains: torch.Tensor = None):
        """The differentiable rollout through the DSLPID loop (`SimCore.rollout_diff_pid`; PID, VEL and ONE_D_PID aviaries): actions
        (K, E, 1, A) -> (obs12 (K,E,1,12), reward (K,E), kin_K [13*ld], pid_K [9,ld], terminated (K,E), truncated (K,E)); the first four
        carry gradients with respect to `actions`, `kin0`, `pid0` (the controller members, `diff.pack_pid`; None: the current ones)
        and `pid_gains` ([6, 3]: replaces the controller's gains for this call -- reading it to the host synchronises -- and receives
        the gradient summed over drones)."""
        obs, reward, kin_k, pid_k, terminated, truncated = self.core.rollout_diff_pid(actions, kin0, pid0, num_steps, pid_gains)
        return obs.view(-1, self.NUM_ENVS, self.NUM_DRONES, 12), reward, kin_k, pid_k, terminated, truncated

    def rollout_policy(self, policy, num_steps: int, noise: torch.Tensor = None, action_std=None, mean_out: torch.Tensor = None):
        """K env steps in ONE launch with the policy in the loop (`policy.MlpPolicy`; the loop of
        `examples/learn.py:157-192`).  The policy's input is the (12,) kinematic row, or -- `full_obs` True / "lazy" and
        `policy.in_dim == 12 + H*A` -- the reference's full row with the action history.  Returns
        `(obs (K,E,1,12), reward (K,E), terminated (K,E), truncated (K,E), actions (K,E,1,A))`.
        `noise` (K,E,1,A) + `action_std` (A): sampled actions for training, `clip(mean + std * noise, -1, 1)`; `mean_out`
        (K,E,1,A) receives the unclipped means (see `SimCore.rollout_policy`)."""
        obs, reward, terminated, truncated, acts = self.core.rollout_policy(policy, num_steps, noise=noise, action_std=action_std,
                                                                            mean_out=mean_out)
        if self.full_obs:
            self.core.history_rows()
        E, D = self.NUM_ENVS, self.NUM_DRONES
        return obs.view(-1, E, D, 12), reward, terminated, truncated, acts.view(-1, E, D, self.ACT_DIM)

    def rollout_mrac(self, ctrl, targets, num_steps: int, last_only: bool = False):
        """K control steps in ONE launch with the adaptive controller in the loop (`SimCore.rollout_mrac`; the loop of the
        reference's `examples/mrac.py:82-90`).  `ctrl`: a `control.VectorMRAC` with one controller per drone; `targets`: (E, 12) /
        (K, E, 12) rows target pos | rpy | vel | rpy rates (rows of 3: positions).  Single-drone aviaries without a task
        (`VectorCtrlAviary`); a plant table (`randomize=` / `set_physical_params`) is honoured.  Returns obs (K, E, 1, 12), or
        (E, 1, 12) with `last_only`."""
        obs = self.core.rollout_mrac(ctrl, targets, num_steps, last_only=last_only)
        return obs.view(-1, self.NUM_ENVS, self.NUM_DRONES, 12) if not last_only else obs.view(self.NUM_ENVS, self.NUM_DRONES, 12)

    def rollout_ctbr(self, ctrl, rows, num_steps: int, mode: str = "cmd", last_only: bool = False, want_cmd: bool = False):
        """K control steps in ONE launch flown on thrust and body-rate commands, the rate loop inside the physics sub-steps
        (`SimCore.rollout_ctbr`).  `ctrl`: a `control.VectorCTBR` with one controller per drone; `rows`: commands (E, 4) / (K, E, 4) in
        `mode="cmd"`, targets (E, 12) / (K, E, 12) (rows of 3: positions) in `mode="pos"`.  Single-drone aviaries without a task
        (`VectorCtrlAviary`); a plant table is honoured.  Returns obs (K, E, 1, 12), or (E, 1, 12) with `last_only`; with `want_cmd` a
        pair (obs, cmd)."""
        out = self.core.rollout_ctbr(ctrl, rows, num_steps, mode=mode, last_only=last_only, want_cmd=want_cmd)
        obs, cmd = out if want_cmd else (out, None)
        obs = obs.view(-1, self.NUM_ENVS, self.NUM_DRONES, 12) if not last_only else obs.view(self.NUM_ENVS, self.NUM_DRONES, 12)
        return (obs, cmd) if want_cmd else obs

    def rollout_diff_ctbr(self, ctrl, rows, kin0: torch.Tensor = None, num_steps: int = None, mode: str = "cmd", gains: torch.Tensor = None):
        """The differentiable rollout on thrust and body-rate commands (`SimCore.rollout_diff_ctbr`): `ctrl`, `rows` and `mode` as in
        `rollout_ctbr` -> (obs12 (K,E,1,12), kin_K [13*ld]), both carrying gradients with respect to `rows`, `kin0` (the plane layout
        of the kinematic state, `diff.pack_kin`; None: the current state) and `gains` ([4, 3]: k_p, k_d, k_rates, k_rate; replaces the
        controller's gains for this call -- reading it to the host synchronises -- and receives the gradient summed over drones)."""
        obs, kin_k = self.core.rollout_diff_ctbr(ctrl, rows, kin0, num_steps, mode, gains)
        return obs.view(-1, self.NUM_ENVS, self.NUM_DRONES, 12), kin_k

    def state_vectors(self) -> torch.Tensor:
        """(E, D, 20) `_getDroneStateVector`-ordered states (needs `track_rpm=True` for the RPM columns)."""
        return self.core.state_vectors().view(self.NUM_ENVS, self.NUM_DRONES, 20)

    # ---- neighbour queries inside every aviary (include/gpd.h gpd_neighbors; envs/BaseAviary.py:658-675) ------------------------
    def _neighbor_query(self, radius, k, rel, want_adjacency):
        if self.NUM_DRONES < 2:
            raise ValueError("neighbour queries need aviaries of at least two drones (num_drones = 1 has nobody to see)")
        radius, k = _nb.check_args(self.NEIGHBOURHOOD_RADIUS if radius is None else radius, k)
        c = self.core
        return _nb.aviary_query(c.kin_P, self.NUM_ENVS, self.NUM_DRONES, radius, k, c._stream(), rel=rel, want_adjacency=want_adjacency)

    def neighbors(self, radius: float = None, k: int = None, rel: bool = True) -> "_nb.Neighbors":
        """For every drone the other drones OF ITS AVIARY closer than `radius` (None: `NEIGHBOURHOOD_RADIUS`): `count` (E, D),
        the nearest `k` (default: min(D - 1, 8)) as `idx` (E, D, k) -- the drone's index inside its aviary, nearest first, ties
        to the lower index, -1 where there are fewer -- and `rel` (E, D, k, 4): relative position and distance.  One launch, no
        host synchronisation."""
        if k is None:
            k = max(1, min(self.NUM_DRONES - 1, 8))
        return self._neighbor_query(radius, k, rel, False)[0]

    def adjacency(self, radius: float = None) -> torch.Tensor:
        """(E, D, D) uint8: `BaseAviary._getAdjacencyMatrix()` (envs/BaseAviary.py:658-675) of every aviary -- 1 on the diagonal
        and where two drones are closer than `radius` (None: `NEIGHBOURHOOD_RADIUS`)."""
        return self._neighbor_query(radius, 1, False, True)[1]

    # ---- obstacle fields (include/gpd.h gpd_obstacles; the reference: BaseAviary._addObstacles, envs/BaseAviary.py:958-981) -----------
    def set_obstacles(self, field: "_ob.ObstacleField", collision_radius: float = None):
        """The obstacles `clearance()` / `range_scan()` / `obstacle_hits()` answer about: one `ObstacleField` shared by every aviary,
        or one with a list per aviary (`ObstacleField(num_envs=E)`); None removes them.  `collision_radius`: the drone as a sphere
        (default: the airframe's `COLLISION_R`).  Nothing acts on the integrator: combine `hit` into your own termination."""
        if field is None:
            self._obstacles = None
            return
        r = self.core.P.COLLISION_R if collision_radius is None else collision_radius
        self._obstacles = _ob.FieldQuery(field, self.device, self.NUM_ENVS * self.NUM_DRONES, self.NUM_DRONES, r)

    def _obstacle_query(self) -> "_ob.FieldQuery":
        q = getattr(self, "_obstacles", None)
        if q is None:
            raise ValueError("no obstacles: call set_obstacles(field) first")
        return q

    def clearance(self) -> "_ob.Clearance":
        """For every drone the nearest obstacle: `normal` (E, D, 3) pointing away from it, the signed `dist` (E, D), its record
        `nearest` (E, D) and `hit` (E, D).  One launch, no host synchronisation; the tensors are reused by the next call."""
        q, c, E, D = self._obstacle_query(), self.core, self.NUM_ENVS, self.NUM_DRONES
        out = q.clearance(c.kin_P, c._stream())
        return _ob.Clearance(out.normal.unflatten(0, (E, D)), out.dist.view(E, D), out.nearest.view(E, D), out.hit.view(E, D))

    def obstacle_hits(self) -> torch.Tensor:
        """(E, D) bool: the drones closer to an obstacle than their collision radius"""
        q, c = self._obstacle_query(), self.core
        return q.hits(c.kin_P, c._stream()).view(self.NUM_ENVS, self.NUM_DRONES)

    def range_scan(self, dirs, max_range: float, frame: str = "body", want_ids: bool = False):
        """(E, D, R) distances along the unit directions `dirs` [R, 3] (`obstacles.fan`; a float32 device tensor is used as it is) to
        the first obstacle, `max_range` where there is none that close.  `frame`: "body" (the directions turn with the attitude),
        "level" (with the yaw only) or "world".  `want_ids`: also the (E, D, R) int32 records that were hit, -1 for none."""
        q, c, E, D = self._obstacle_query(), self.core, self.NUM_ENVS, self.NUM_DRONES
        ranges, ids = q.scan(c.kin_P, c.kin_Q, dirs, max_range, frame, want_ids, c._stream())
        return (ranges.view(E, D, -1), ids.view(E, D, -1)) if want_ids else ranges.view(E, D, -1)

    # ---- sampling-based MPC (include/gpd.h gpd_mppi; the reference has no planner) ---------------------------------------------------
    def mppi(self, horizon: int, samples: int, sigma, lam: float, cost: "_mppi.MPPICost" = None, seed: int = 0, act_lo=None,
             act_hi=None, model: str = "nominal", plant=None) -> "_mppi.MPPI":
        """An `mppi.MPPI` planner bound to this batch (single drones, RPM or VEL actions) and to the field given to `set_obstacles()`,
        if any: `plan(goal)` returns the next action `(E, 4)` from the current state, `advance()` shifts the nominal after it was
        flown.  The default bounds are [-1, 1]^4 for RPM and [-1, 1]^3 x [0, 1] for VEL.  `model="nominal"`: the planning model is
        the flag-less DYN integrator of the nominal airframe, whatever this batch flies; `model="aviary"`: this batch's `physics` flags
        and its per-drone airframes as they are at each plan (`randomize=`, `set_physical_params`), or the belief `plant`."""
        return _mppi.MPPI(self.core, horizon, samples, sigma, lam, cost=cost, seed=seed, field=getattr(self, "_obstacles", None),
                          act_lo=act_lo, act_hi=act_hi, model=model, plant=plant)

    def mppi_ctbr(self, ctrl, horizon: int, samples: int, sigma, lam: float, cost: "_mppi.MPPICost" = None, seed: int = 0, act_lo=None,
                  act_hi=None, model: str = "nominal", plant=None) -> "_mppi.CTBRMPPI":
        """An `mppi.CTBRMPPI` planner over thrust and body-rate commands bound to this batch (single drones, RPM actions:
        `VectorCtrlAviary`), to `ctrl` (a `control.VectorCTBR` with one controller per drone) and to the field given to
        `set_obstacles()`, if any: `plan(goal)` returns `(E, 4)` commands for `rollout_ctbr(ctrl, cmd, 1, mode="cmd")`.  The default
        bounds are the controller's clips.  `model`, `plant`: as for `mppi()`."""
        return _mppi.CTBRMPPI(self.core, ctrl, horizon, samples, sigma, lam, cost=cost, seed=seed, field=getattr(self, "_obstacles", None),
                              act_lo=act_lo, act_hi=act_hi, model=model, plant=plant)

    def mppi_swarm(self, horizon: int, samples: int, sigma, lam: float, cost: "_mppi.MPPICost" = None, seed: int = 0, ctrl=None, k: int = 8,
                   radius: float = None, w_peer: float = 100.0, peer_dist: float = None, intruders: int = 0, box=None, act_lo=None,
                   act_hi=None) -> "_mppi.SwarmMPPI":
        """An `mppi.SwarmMPPI` planner bound to this batch and to the field given to `set_obstacles()`, if any: `mppi()` (or, with
        `ctrl`, `mppi_ctbr()`) for single drones that SHARE ONE AIRSPACE -- every drone's cost also keeps it `peer_dist` away from
        where its `k` nearest peers last published they would be, and every plan publishes the drone's own path (`gpd_mppi_peers`,
        one launch per plan)."""
        return _mppi.SwarmMPPI(self.core, horizon, samples, sigma, lam, cost=cost, seed=seed, field=getattr(self, "_obstacles", None), ctrl=ctrl,
                               k=k, radius=radius, w_peer=w_peer, peer_dist=peer_dist, intruders=intruders, box=box, act_lo=act_lo, act_hi=act_hi)

    # ---- domain randomisation: the plant of every drone (include/gpd.h GPD_SCALE_*; SimCore.set_plant) ------------------------
    def set_physical_params(self, mask=None, **scales):
        """Scale the plant of every drone (or of the aviaries in the bool/uint8 `mask` [E]) relative to the nominal airframe:
        fields of `_native.SCALE_FIELDS` (mass, ixx, iyy, izz, kf, km, drag_xy, drag_z, gnd_eff), each a scalar, an [E] or an [E, D]
        tensor of finite factors > 0; fields left out keep their values.  The plant changes; what the agent and the controller know
        does not: the action mapping (HOVER_RPM, the MAX_RPM clip), DSLPID's model and gains, SPEED_LIMIT, the geometry and the task
        stay nominal -- a drone with mass 1.2 that receives action 0 sinks.  All factors 1.0 is the nominal airframe bit for bit."""
        self.core.set_plant(scales, mask=mask)

    def physical_params(self) -> torch.Tensor:
        """(E, D, 9) scale factors of every drone's plant, in `_native.SCALE_FIELDS` order (privileged / asymmetric-critic inputs):
        a VIEW of the table when there is one, else ones."""
        v = self.core.plant_view()
        if v is None:
            return torch.ones((self.NUM_ENVS, self.NUM_DRONES, len(_native.SCALE_FIELDS)), dtype=torch.float32, device=self.device)
        return v.permute(1, 2, 0)

    @staticmethod
    def _check_randomize(randomize):
        if not randomize:
            return {}
        out = {}
        for k, r in dict(randomize).items():
            if k not in _native.SCALE_FIELDS:
                raise ValueError(f"randomize: unknown field {k!r} (fields: {', '.join(_native.SCALE_FIELDS)})")
            r = float(r)
            if not (math.isfinite(r) and 0.0 <= r < 1.0):
                raise ValueError(f"randomize: the range of {k} must satisfy 0 <= r < 1, got {r}")
            out[k] = r
        return out

    def _resample(self, mask):
        """New scales U(1 - r, 1 + r) for the randomised fields of the aviaries in `mask` (None: all): one torch.rand and one
        gpd_plant_derive, no host sync."""
        E, D = self.NUM_ENVS, self.NUM_DRONES
        cur = self.core.plant_view()
        full = cur.clone() if cur is not None else torch.ones((len(_native.SCALE_FIELDS), E, D), dtype=torch.float32, device=self.device)
        u = torch.rand((len(self.randomize), E, D), generator=self._rng, device=self.device)
        for i, (k, r) in enumerate(self.randomize.items()):
            full[_native.SCALE_FIELDS.index(k)] = 1.0 + r * (2.0 * u[i] - 1.0)
        self.core._apply_plant(full, mask)

    # ---- checkpoint / resume; non-finite guard (both absent upstream) ----------------------
    def get_state(self) -> dict:
        """Complete snapshot (device clones): integrator state, controller members, episode clocks, latest observations and -- with
        `full_obs` -- the action ring and its positions.  `set_state(get_state())` resumes bit for bit, history tails included."""
        return self.core.get_state()

    def set_state(self, state: dict):
        self.core.set_state(**state)
        if self.full_obs:                    # the materialised rows follow from obs12 + ring
            self.core.history_rows()
        return self._obs()

    def bad_envs(self) -> torch.Tensor:
        """[E] bool device tensor: aviaries whose state holds a NaN / infinity after the latest step (`nan_guard=True`)."""
        return self.core.bad_envs()

    def close(self):
        pass


class VectorHoverAviary(VectorAviary):
    """E x `HoverAviary` (one drone each)."""

    def __init__(self, num_envs: int, drone_model: DroneModel = DroneModel.CF2X, initial_xyzs=None, initial_rpys=None,
                 physics: Physics = Physics.DYN, pyb_freq: int = 240, ctrl_freq: int = 30,
                 obs: ObservationType = ObservationType.KIN, act: ActionType = ActionType.RPM, **kw):
        super().__init__(num_envs=num_envs, num_drones=1, drone_model=drone_model, initial_xyzs=initial_xyzs,
                         initial_rpys=initial_rpys, physics=physics, pyb_freq=pyb_freq, ctrl_freq=ctrl_freq, obs=obs,
                         act=act, task="hover", **kw)


class VectorMultiHoverAviary(VectorAviary):
    """E x `MultiHoverAviary` (`num_drones` drones each, default 2)."""

    def __init__(self, num_envs: int, num_drones: int = 2, drone_model: DroneModel = DroneModel.CF2X,
                 initial_xyzs=None, initial_rpys=None, physics: Physics = Physics.DYN, pyb_freq: int = 240,
                 ctrl_freq: int = 30, obs: ObservationType = ObservationType.KIN, act: ActionType = ActionType.RPM, **kw):
        super().__init__(num_envs=num_envs, num_drones=num_drones, drone_model=drone_model, initial_xyzs=initial_xyzs,
                         initial_rpys=initial_rpys, physics=physics, pyb_freq=pyb_freq, ctrl_freq=ctrl_freq, obs=obs,
                         act=act, task="multihover", **kw)


class VectorCtrlAviary(VectorAviary):
    """E x `CtrlAviary`: raw RPM actions clipped to [0, MAX_RPM], no task."""

    def __init__(self, num_envs: int, num_drones: int = 1, drone_model: DroneModel = DroneModel.CF2X,
                 initial_xyzs=None, initial_rpys=None, physics: Physics = Physics.DYN, pyb_freq: int = 240,
                 ctrl_freq: int = 240, **kw):
        kw.setdefault("auto_reset", False)
        kw.setdefault("track_rpm", True)
        super().__init__(num_envs=num_envs, num_drones=num_drones, drone_model=drone_model, initial_xyzs=initial_xyzs,
                         initial_rpys=initial_rpys, physics=physics, pyb_freq=pyb_freq, ctrl_freq=ctrl_freq,
                         act="raw_rpm", task="none", **kw)


class VectorVelocityAviary(VectorAviary):
    """E x `VelocityAviary`: velocity commands `[vx, vy, vz, fraction of SPEED_LIMIT]` tracked by the embedded DSLPID
    controllers (`GPD_ACT_VEL`), no task; `state_vectors()` gives the (E, D, 20) observation of the reference class."""

    def __init__(self, num_envs: int, num_drones: int = 1, drone_model: DroneModel = DroneModel.CF2X,
                 initial_xyzs=None, initial_rpys=None, physics: Physics = Physics.DYN, pyb_freq: int = 240,
                 ctrl_freq: int = 240, **kw):
        kw.setdefault("auto_reset", False)
        kw.setdefault("track_rpm", True)
        super().__init__(num_envs=num_envs, num_drones=num_drones, drone_model=drone_model, initial_xyzs=initial_xyzs,
                         initial_rpys=initial_rpys, physics=physics, pyb_freq=pyb_freq, ctrl_freq=ctrl_freq,
                         act=ActionType.VEL, task="none", **kw)


class VectorObstacleAviary(VectorAviary):
    """E single-drone aviaries flying an obstacle course AS A TASK: contact with the `field` is scored and (by default) ends the episode,
    a proximity hinge shapes the reward, and the observation row carries the nearest obstacle and a range-sensor fan --
    `(E, 1, 16 + R)`: pos rpy vel ang_v | nx ny nz d | range_0 .. range_{R-1}.  One launch per `step()` and one per K-step
    `rollout()` (`gpd_rollout_obst`): the collision test, the reset it triggers and the scan of the pose that is observed all happen
    inside the step kernel.  The reference gestures at this with `BaseRLAviary._addObstacles` and never scores it.

    `field`: an `obstacles.ObstacleField`, shared or one list per aviary.  `rays`: `[R, 3]` unit directions (`obstacles.fan(16, ...)`) or
    None; `max_range`, `frame` ("body", "level", "world") as in `range_scan()`.  reward = the task's reward + `hit_reward` in the step
    that ends in contact - `prox_weight` * max(0, `prox_margin` - gap), gap the distance left before contact; `collision_radius`: the
    drone as a sphere (default: the airframe's COLLISION_R).  There is no collision response: with `hit_terminates=False` a drone flies
    on through the obstacle.  Terminal observations and the action history are not kept.  What `step()` and `rollout()` return are views of
    buffers that the next call overwrites."""

    def __init__(self, num_envs: int, field: "_ob.ObstacleField", rays=None, max_range: float = 5.0, frame: str = "body",
                 hit_terminates: bool = True, hit_reward: float = -1.0, prox_margin: float = 0.0, prox_weight: float = 0.0,
                 collision_radius: float = None, act=ActionType.VEL, task: str = "hover", target_pos=None, num_drones: int = 1,
                 drone_model: DroneModel = DroneModel.CF2X, initial_xyzs=None, initial_rpys=None, physics: Physics = Physics.DYN,
                 pyb_freq: int = 240, ctrl_freq: int = 48, episode_len_sec: float = 8, auto_reset: bool = True, full_obs: bool = False,
                 keep_terminal_obs: bool = False, track_rpm: bool = False, pyb_like: bool = None, nan_guard: bool = False,
                 randomize: dict = None, device=None):
        self._refuse(num_drones, act, task, physics, pyb_like, full_obs, keep_terminal_obs, nan_guard, randomize)
        rays = self.check_rays(rays)
        n_rays = 0 if rays is None else len(rays)
        if field.num_envs is not None and field.num_envs != int(num_envs):
            raise ValueError(f"the field has a list for each of {field.num_envs} aviaries; the simulation has {int(num_envs)}")
        r = DroneParams(drone_model).COLLISION_R if collision_radius is None else collision_radius
        self._task = self.task_struct(r, hit_terminates, hit_reward, prox_margin, prox_weight, n_rays, frame, max_range)    # (before any device work)
        super().__init__(num_envs=num_envs, num_drones=1, drone_model=drone_model, initial_xyzs=initial_xyzs, initial_rpys=initial_rpys,
                         physics=physics, pyb_freq=pyb_freq, ctrl_freq=ctrl_freq, act=act, task=task, target_pos=target_pos,
                         episode_len_sec=episode_len_sec, auto_reset=auto_reset, track_rpm=track_rpm, pyb_like=pyb_like, device=device)
        self.N_RAYS, self.MAX_RANGE, self.FRAME = n_rays, float(max_range), frame
        self.OBS_DIM = 16 + n_rays
        self.ROW_LD = (self.OBS_DIM + 3) // 4 * 4
        self._rays = None if rays is None else torch.as_tensor(rays).to(self.device).contiguous()
        self._obstacles = _ob.FieldQuery(field, self.device, self.NUM_ENVS, 1, r)        # (also what clearance() / range_scan() answer about)
        self._row = torch.zeros((self.NUM_ENVS, self.ROW_LD), dtype=torch.float32, device=self.device)
        self._latest = self._row
        self.collided = torch.zeros(self.NUM_ENVS, dtype=torch.bool, device=self.device)
        self._fill_rows(None)

    @staticmethod
    def _refuse(num_drones, act, task, physics, pyb_like, full_obs, keep_terminal_obs, nan_guard, randomize):
        """what the obstacle task does not serve (include/gpd.h gpd_rollout_obst), before any device work"""
        if int(num_drones) != 1:
            raise NotImplementedError("VectorObstacleAviary: num_drones > 1 (an obstacle course is flown by single drones)")
        for name, value in (("randomize", randomize), ("full_obs", full_obs), ("keep_terminal_obs", keep_terminal_obs), ("nan_guard", nan_guard)):
            if value:
                raise NotImplementedError(f"VectorObstacleAviary: {name} is not served by the fused obstacle task")
        if act not in (ActionType.RPM, ActionType.VEL, ActionType.PID):
            raise NotImplementedError("VectorObstacleAviary: act must be ActionType.RPM, ActionType.VEL or ActionType.PID")
        if task not in ("hover", "none"):
            raise NotImplementedError("VectorObstacleAviary: task must be 'hover' or 'none'")
        flags = physics.mask(pyb_like) if isinstance(physics, Physics) else int(physics)
        if flags & 4:
            raise NotImplementedError("VectorObstacleAviary: downwash needs mates, the course is flown alone")

    @staticmethod
    def check_rays(rays):
        """`rays` as a contiguous float32 `[R, 3]` array, 1 <= R <= 64 (None stays None)"""
        if rays is None:
            return None
        rays = np.ascontiguousarray(rays.cpu().numpy() if isinstance(rays, torch.Tensor) else rays, dtype=np.float32)
        if rays.ndim != 2 or rays.shape[1] != 3 or not 1 <= rays.shape[0] <= _ob.MAX_RAYS:
            raise ValueError(f"rays must be [1..{_ob.MAX_RAYS}, 3] unit vectors or None, got {rays.shape}")
        return rays

    @staticmethod
    def task_struct(collision_radius, hit_terminates, hit_reward, prox_margin, prox_weight, n_rays, frame, max_range) -> "_native.GpdObstTask":
        """the `GpdObstTask` of the arguments; ValueError for what `gpd_rollout_obst` would refuse"""
        code = _ob.FRAMES.get(frame)
        if code is None:
            raise ValueError(f"frame must be one of {', '.join(_ob.FRAMES)}, got {frame!r}")
        vals = dict(collision_radius=float(collision_radius), hit_reward=float(hit_reward), prox_margin=float(prox_margin),
                    prox_weight=float(prox_weight), max_range=float(max_range))
        if not all(math.isfinite(v) for v in vals.values()):
            raise ValueError(f"collision_radius, hit_reward, prox_margin, prox_weight and max_range must be finite, got {vals}")
        if not vals["collision_radius"] > 0.0 or not vals["max_range"] > 0.0:
            raise ValueError("collision_radius and max_range must be positive")
        if vals["prox_margin"] < 0.0 or vals["prox_weight"] < 0.0:
            raise ValueError("prox_margin and prox_weight must be non-negative")
        return _native.GpdObstTask(hit_terminates=int(bool(hit_terminates)), n_rays=int(n_rays), ray_frame=code, **vals)

    def _obs(self):
        return self._latest.view(self.NUM_ENVS, 1, self.ROW_LD)[..., :self.OBS_DIM]

    def _fill_rows(self, mask):
        """the rows of the poses a reset left, from the existing entries (gpd_obstacles; reset is not hot)"""
        c, q = self.core, self._obstacles
        new = torch.zeros_like(self._row)
        new[:, :12] = c.obs12
        q.clearance(c.kin_P, c._stream())
        new[:, 12:16] = q._clear4
        if self.N_RAYS:
            new[:, 16:self.OBS_DIM] = q.scan(c.kin_P, c.kin_Q, self._rays, self.MAX_RANGE, self.FRAME, False, c._stream())[0]
        if mask is None:
            self._row.copy_(new)
        else:
            keep = self._latest
            torch.where(mask.to(device=self.device, dtype=torch.bool).unsqueeze(1), new, keep, out=self._row)
        self._latest = self._row

    def reset(self, seed=None, options=None, mask=None):
        """Reset all aviaries (or those of the bool/uint8 `mask` [E]); the rows of the reset poses carry their clearance and ranges."""
        self.core.reset(mask=mask)
        self._fill_rows(mask)
        return self._obs(), {}

    def _launch(self, actions, num_steps, last_only):
        q = self._obstacles
        return self.core.rollout_obst(self._task, q.obst, q.n_obst, q.obst_ld, self._rays, actions, num_steps=num_steps, last_only=last_only)

    def step(self, action: torch.Tensor):
        """action (E, 1, A) -> (obs (E, 1, 16 + R), reward [E], terminated [E], truncated [E], {"collided": (E,) bool}): ONE launch.
        Everything returned -- `info["collided"]` and `self.collided` included -- is a VIEW of the core's persistent output buffers:
        the next `step()` overwrites it.  `clone()` what has to outlive the next call."""
        rows, reward, terminated, truncated, collided = self._launch(action, 1, True)
        self._latest = rows[0]
        self.collided = collided[0]
        return self._obs(), reward[0], terminated[0], truncated[0], {"collided": collided[0]}

    def rollout(self, actions: torch.Tensor):
        """actions (K, E, 1, A) -> (obs (K, E, 1, 16 + R), reward (K, E), terminated (K, E), truncated (K, E), {"collided": (K, E)}):
        K steps in ONE launch, bit for bit K calls of `step()`.  Views of persistent buffers, as in `step()`: the next `rollout()` of
        the same K overwrites them."""
        K = actions.shape[0]
        rows, reward, terminated, truncated, collided = self._launch(actions, None, False)
        self._latest = rows[K - 1]
        self.collided = collided[K - 1]
        return rows.view(K, self.NUM_ENVS, 1, self.ROW_LD)[..., :self.OBS_DIM], reward, terminated, truncated, {"collided": collided}

    def set_obstacles(self, field, collision_radius: float = None):
        raise NotImplementedError("VectorObstacleAviary: the field is part of the task, given at construction")


class VectorCTBRAviary(VectorAviary):
    """E single-drone aviaries whose ACTION is the thrust and body-rate command (CTBR), the action space agile-flight RL trains on:
    `obs, r, term, trunc, info = env.step(a)` with `a (E, 1, 4)` in [-1, 1], a body-rate loop closed inside every physics sub-step in
    place of the firmware (`control.VectorCTBR`, owned by the aviary as `ctrl`).  One launch per `step()` and one per K-step `rollout()`
    (`gpd_rollout_ctbr_task`): the rate loop, the task's reward and flags, the same-step auto-reset and the terminal observation all
    happen inside the kernel.

    `normalized=True` (default): thrust = `thrust_center + a_0 thrust_span`, rates = `a_{1..3} rate_span`, hover-centred by default --
    center = span = the controller's g (9.8 m/s^2: `a = 0` is the hover command, `a = -1` zero thrust), rate_span = the controller's
    `rate_max`.  `normalized=False`: the action is the physical command (thrust [m/s^2] | rates [rad/s]).  Either way the rate loop's
    `thrust_max` / `rate_max` clips bound what is flown.  `randomize`, `keep_terminal_obs`, `nan_guard`, `reset(mask=)`: as in
    `VectorAviary`.  Not served: aviaries of several drones, the action history (`full_obs`), downwash, position targets as the
    action."""

    def __init__(self, num_envs: int, thrust_center: float = None, thrust_span: float = None, rate_span: float = None, normalized: bool = True,
                 k_rate=None, thrust_max: float = None, rate_max: float = None, ctrl_freq: int = 48, task: str = "hover", target_pos=None,
                 num_drones: int = 1, drone_model: DroneModel = DroneModel.CF2X, initial_xyzs=None, initial_rpys=None,
                 physics: Physics = Physics.DYN, pyb_freq: int = 240, episode_len_sec: float = 8, auto_reset: bool = True,
                 full_obs: bool = False, keep_terminal_obs: bool = False, track_rpm: bool = False, pyb_like: bool = None,
                 nan_guard: bool = False, randomize: dict = None, device=None):
        from ..control.CTBRControl import K_RATE, RATE_MAX, THRUST_MAX, VectorCTBR, to_struct
        self._refuse(num_drones, task, physics, pyb_like, full_obs)
        k_rate = K_RATE if k_rate is None else k_rate
        thrust_max = THRUST_MAX if thrust_max is None else thrust_max
        rate_max = RATE_MAX if rate_max is None else rate_max
        gains = to_struct(DroneParams(drone_model), k_rate, thrust_max, rate_max)     # (ValueError for bad gains, before any device work)
        self._task = self.task_struct(gains.g, gains.rate_max, thrust_center, thrust_span, rate_span, normalized)
        super().__init__(num_envs=num_envs, num_drones=1, drone_model=drone_model, initial_xyzs=initial_xyzs, initial_rpys=initial_rpys,
                         physics=physics, pyb_freq=pyb_freq, ctrl_freq=ctrl_freq, act="raw_rpm", task=task, target_pos=target_pos,
                         episode_len_sec=episode_len_sec, auto_reset=auto_reset, keep_terminal_obs=keep_terminal_obs, track_rpm=track_rpm,
                         pyb_like=pyb_like, nan_guard=nan_guard, randomize=randomize, device=device)
        self.ctrl = VectorCTBR(self.NUM_ENVS, drone_model, device=self.device, k_rate=k_rate, thrust_max=thrust_max, rate_max=rate_max)
        self.NORMALIZED = bool(normalized)
        self.ACT_DIM, self.OBS_DIM = 4, 12

    @staticmethod
    def _refuse(num_drones, task, physics, pyb_like, full_obs):
        """what the fused CTBR task does not serve (include/gpd.h gpd_rollout_ctbr_task), before any device work"""
        if int(num_drones) != 1:
            raise NotImplementedError("VectorCTBRAviary: num_drones > 1 (the command flies a single drone)")
        if full_obs:
            raise NotImplementedError("VectorCTBRAviary: full_obs (the action history) is not served by the fused CTBR task")
        if task not in ("hover", "none"):
            raise NotImplementedError("VectorCTBRAviary: task must be 'hover' or 'none'")
        flags = physics.mask(pyb_like) if isinstance(physics, Physics) else int(physics)
        if flags & 4:
            raise NotImplementedError("VectorCTBRAviary: downwash needs mates, the command flies a single drone")

    @staticmethod
    def task_struct(g, rate_max, thrust_center=None, thrust_span=None, rate_span=None, normalized=True) -> "_native.GpdCtbrTask":
        """the `GpdCtbrTask` of the arguments: cmd = (thrust_center + a_0 thrust_span, a_1 rate_span, a_2 rate_span, a_3 rate_span), the
        defaults hover-centred (center = span = `g`, rate_span = `rate_max`); ValueError for values that are not finite"""
        center = float(g) if thrust_center is None else float(thrust_center)
        span = float(g) if thrust_span is None else float(thrust_span)
        rspan = float(rate_max) if rate_span is None else float(rate_span)
        if not all(math.isfinite(v) for v in (center, span, rspan)):
            raise ValueError(f"thrust_center, thrust_span and rate_span must be finite, got {(center, span, rspan)}")
        t = _native.GpdCtbrTask(normalized=int(bool(normalized)))
        t.act_scale[0], t.act_bias[0] = span, center
        for i in (1, 2, 3):
            t.act_scale[i], t.act_bias[i] = rspan, 0.0
        return t

    def command(self, action: torch.Tensor) -> torch.Tensor:
        """the physical command (thrust [m/s^2] | rates [rad/s]) of `action`, in its shape: the kernel's map as torch operations (a
        diagnostic; rounds once more than the kernel's fused multiply-add)"""
        if not self.NORMALIZED:
            return action
        scale = torch.tensor(list(self._task.act_scale), dtype=torch.float32, device=action.device)
        bias = torch.tensor(list(self._task.act_bias), dtype=torch.float32, device=action.device)
        return action * scale + bias

    def action_of(self, cmd: torch.Tensor) -> torch.Tensor:
        """the action whose command is `cmd` (the inverse of the map, not clipped to [-1, 1])"""
        if not self.NORMALIZED:
            return cmd
        scale = torch.tensor(list(self._task.act_scale), dtype=torch.float32, device=cmd.device)
        bias = torch.tensor(list(self._task.act_bias), dtype=torch.float32, device=cmd.device)
        return (cmd - bias) / scale

    def step(self, action: torch.Tensor):
        """action (E, 1, 4) -> (obs (E, 1, 12), reward [E], terminated [E], truncated [E], info): ONE launch.  With `keep_terminal_obs`,
        `info["terminal_observation"]` holds the last row of every episode that ended."""
        _, reward, terminated, truncated = self.core.rollout_ctbr_task(self.ctrl, action, 1, last_only=True, task=self._task)
        if self.randomize and self.core.auto_reset:          # the aviaries that ended were reset by the step: new airframes
            self._resample(terminated | truncated)
        info = {}
        if self.core.term_obs12 is not None:
            info["terminal_observation"] = self.core.term_obs12.view(self.NUM_ENVS, 1, 12)
        return self._obs(), reward, terminated, truncated, info

    def rollout(self, actions: torch.Tensor):
        """actions (K, E, 1, 4) -> (obs (K, E, 1, 12), reward (K, E), terminated (K, E), truncated (K, E)): K steps in ONE launch, bit for
        bit K calls of `step()` (with `randomize`, an aviary that ends inside the launch keeps its airframe until the launch ends)."""
        K = actions.shape[0]
        obs, reward, terminated, truncated = self.core.rollout_ctbr_task(self.ctrl, actions, task=self._task)
        if self.randomize and self.core.auto_reset:
            self._resample((terminated | truncated).any(dim=0))
        return obs.view(K, self.NUM_ENVS, 1, 12), reward, terminated, truncated


class VecEnvAdapter:
    """Stable-Baselines3 `VecEnv`-shaped front end of a `VectorAviary` (duck-typed: SB3 is not installed here).

    Follows `DummyVecEnv` (what `examples/learn.py:54-58` builds through `make_vec_env`): numpy in / numpy out,
    `dones = terminated | truncated`, aviaries that end are reset inside the same `step_wait()` and report the
    last observation of the finished episode as `infos[i]["terminal_observation"]` together with
    `infos[i]["TimeLimit.truncated"]`.  Observations are `(num_envs, D, 12 [+ H*A])` (squeezed to
    `(num_envs, 12 [+ H*A])` for one drone per aviary when `squeeze=True`).  The device tensors of the last step
    stay available as `last` for a GPU-resident learner that does not want the host copies.
    """

    def __init__(self, env: "VectorAviary", squeeze: bool = False):
        if not env.core.auto_reset:
            raise ValueError("VecEnvAdapter needs a VectorAviary built with auto_reset=True")
        self.env = env
        self.num_envs = env.NUM_ENVS
        self.squeeze = bool(squeeze and env.NUM_DRONES == 1)
        from .._gym_shim import spaces
        D, W, A = env.NUM_DRONES, env.OBS_DIM, env.ACT_DIM
        oshape, ashape = ((W,), (A,)) if self.squeeze else ((D, W), (D, A))
        self.observation_space = spaces.Box(low=np.full(oshape, -np.inf), high=np.full(oshape, np.inf), dtype=np.float32)
        self.action_space = spaces.Box(low=-np.ones(ashape), high=np.ones(ashape), dtype=np.float32)
        self._actions = None
        self.last = None
        if env.core.term_obs12 is None:     # terminal observations are part of the VecEnv contract
            env.core.term_obs12 = torch.zeros((env.core.N, 12), dtype=torch.float32, device=env.device)

    def _np_obs(self, obs):
        o = obs.cpu().numpy()
        return o[:, 0, :] if self.squeeze else o

    def reset(self):
        obs, _ = self.env.reset()
        return self._np_obs(obs)

    def step_async(self, actions):
        a = torch.as_tensor(np.asarray(actions, dtype=np.float32), device=self.env.device)
        self._actions = a.reshape(self.num_envs, self.env.NUM_DRONES, self.env.ACT_DIM)

    def step_wait(self):
        env = self.env
        obs, reward, terminated, truncated, _ = env.step(self._actions)
        self.last = (obs, reward, terminated, truncated)
        packed = torch.stack([reward, terminated.to(torch.float32), truncated.to(torch.float32)]).cpu().numpy()
        rew, term, trunc = packed[0], packed[1] != 0, packed[2] != 0
        dones = term | trunc
        infos = [{} for _ in range(self.num_envs)]
        idx = np.flatnonzero(dones)
        if idx.size:
            tobs = env.core.term_obs12.view(self.num_envs, env.NUM_DRONES, 12)[torch.as_tensor(idx, device=env.device)].cpu().numpy()
            if env.full_obs:    # the history tail of the terminal observation is the one of the returned row
                tail = obs[torch.as_tensor(idx, device=env.device)][..., 12:].cpu().numpy()
                tobs = np.concatenate([tobs, tail], axis=-1)
            for j, i in enumerate(idx):
                infos[i]["terminal_observation"] = tobs[j, 0] if self.squeeze else tobs[j]
                infos[i]["TimeLimit.truncated"] = bool(trunc[i] and not term[i])
        return self._np_obs(obs), rew, dones, infos

    def step(self, actions):
        self.step_async(actions)
        return self.step_wait()

    def close(self):
        self.env.close()

    def get_attr(self, name, indices=None):
        n = self.num_envs if indices is None else len(np.atleast_1d(indices))
        return [getattr(self.env, name)] * n

    def env_is_wrapped(self, wrapper_class, indices=None):
        n = self.num_envs if indices is None else len(np.atleast_1d(indices))
        return [False] * n

    def seed(self, seed=None):
        return [seed] * self.num_envs          # the simulator is deterministic: nothing draws random numbers


class GymVectorEnvAdapter:
    """`gymnasium.vector.VectorEnv`-shaped front end of a `VectorAviary` (duck-typed: gymnasium is optional here).

    The gymnasium >= 1.0 vector API (what `gymnasium.make_vec` / `SyncVectorEnv` give a learner that does not go through
    SB3's `make_vec_env`, `examples/learn.py:54-58`): `reset(seed=, options=) -> (obs, infos)`, `step(actions) ->
    (obs, rewards, terminations, truncations, infos)` with batched numpy arrays, `num_envs`, `single_observation_space`
    / `single_action_space` and their batched versions, and an explicit autoreset mode.  The kernel resets an aviary in
    the SAME step it ends in (`AutoresetMode.SAME_STEP`): the returned observation is the first one of the new episode
    and the last one of the finished episode is `infos["final_obs"][i]` (with the mask `infos["_final_obs"]`), as
    gymnasium's own same-step vector envs report it.  `last` keeps the device tensors of the latest step for a
    GPU-resident learner."""

    metadata = {"autoreset_mode": "SameStep", "render_modes": []}

    def __init__(self, env: "VectorAviary"):
        if not env.core.auto_reset:
            raise ValueError("GymVectorEnvAdapter needs a VectorAviary built with auto_reset=True")
        self.env = env
        self.num_envs = env.NUM_ENVS
        from .._gym_shim import spaces
        D, W, A = env.NUM_DRONES, env.OBS_DIM, env.ACT_DIM
        box = lambda shape, lo, hi: spaces.Box(low=np.full(shape, lo), high=np.full(shape, hi), dtype=np.float32)  # noqa: E731
        self.single_observation_space = box((D, W), -np.inf, np.inf)
        self.single_action_space = box((D, A), -1.0, 1.0)
        self.observation_space = box((self.num_envs, D, W), -np.inf, np.inf)
        self.action_space = box((self.num_envs, D, A), -1.0, 1.0)
        self.last = None
        self.closed = False
        if env.core.term_obs12 is None:
            env.core.term_obs12 = torch.zeros((env.core.N, 12), dtype=torch.float32, device=env.device)

    def reset(self, *, seed=None, options=None):
        mask = None if not options or "reset_mask" not in options else torch.as_tensor(options["reset_mask"], device=self.env.device)
        obs, _ = self.env.reset(seed=seed, mask=mask)
        return obs.cpu().numpy(), {}

    def step(self, actions):
        env = self.env
        a = torch.as_tensor(np.asarray(actions, dtype=np.float32), device=env.device).reshape(self.num_envs, env.NUM_DRONES, env.ACT_DIM)
        obs, reward, terminated, truncated, _ = env.step(a)
        self.last = (obs, reward, terminated, truncated)
        packed = torch.stack([reward, terminated.to(torch.float32), truncated.to(torch.float32)]).cpu().numpy()
        rew, term, trunc = packed[0], packed[1] != 0, packed[2] != 0
        obs_np = obs.cpu().numpy()
        infos = {}
        done = term | trunc
        if done.any():
            final = np.zeros_like(obs_np)
            tob = env.core.term_obs12.view(self.num_envs, env.NUM_DRONES, 12).cpu().numpy()
            final[done, :, :12] = tob[done]
            final[done, :, 12:] = obs_np[done, :, 12:]       # the history tail is not cleared by a reset (App. B.2)
            infos["final_obs"], infos["_final_obs"] = final, done
        return obs_np, rew, term, trunc, infos

    def close(self, **kwargs):
        self.closed = True
        self.env.close()

    def render(self):
        return None

    @property
    def unwrapped(self):
        return self
