/*
 * gpd.h — C-ABI of libgpd.so, the MI355X (gfx950) native hot path of the vectorised
 * quadrotor simulator: BaseAviary's per-drone physics step (explicit integrator + drag,
 * ground effect, downwash), DSLPIDControl, the RL action mapping, the 12-float kinematic
 * observation and the Hover / MultiHover reward, termination and truncation tests, fused
 * into one HIP kernel over a structure-of-arrays drone state.
 *
 * The reference (utiasDSL/gym-pybullet-drones, pure Python) has no FFI layer; its boundary is
 * the Python class surface.  Each entry point below names the reference code it replaces
 * (paths relative to the reference checkout, gym_pybullet_drones/...).  INTEGRATION.md shows
 * the ctypes binding a reference maintainer would add.
 *
 * Conventions
 *   - every pointer is a DEVICE pointer into caller-owned memory (PyTorch-ROCm tensors on the
 *     Python side); the library never allocates, frees or retains tensor memory;
 *   - every call is asynchronous on the hipStream_t passed as `void* stream` (NULL = default
 *     stream), takes no locks and keeps no mutable global state except the thread-local
 *     last-error string, so it is re-entrant per stream and capturable in a hipGraph;
 *   - return value: 0 on success, a negative GPD_E* code for argument errors, a positive
 *     hipError_t for runtime errors; gpd_last_error() describes the last failure of the
 *     calling thread.  No C++ exception crosses the boundary;
 *   - drone n = env * drones_per_env + d (the D drones of one aviary are adjacent);
 *   - quaternions are (x, y, z, w), as in the reference's state vector
 *     (envs/BaseAviary.py:559);
 *   - all arithmetic is fp32, no -ffast-math; FP contraction is off and every fused multiply-add is explicit in the
 *     source, so a drone's trajectory is bit-identical in every kernel variant (gpd_step vs gpd_rollout, aviary
 *     size, batch size, lane); reciprocals/square roots are the 1-ulp hardware instructions and
 *     atan2/asin/sin/cos are <= 2-ulp polynomials (csrc/gpd_common.inc).
 */
#ifndef GPD_H
#define GPD_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define GPD_ABI_VERSION 9

/* DroneModel (utils/enums.py:3-8) */
enum { GPD_MODEL_CF2X = 0, GPD_MODEL_CF2P = 1, GPD_MODEL_RACE = 2 };

/* ActionType (utils/enums.py:35-41) + the raw, clipped RPM action of CtrlAviary
 * (envs/CtrlAviary.py:121-140) */
enum {
    GPD_ACT_RPM = 0,       /* rpm = HOVER_RPM*(1+0.05*a[0:4])      envs/BaseRLAviary.py:191-192 */
    GPD_ACT_PID = 1,       /* a[0:3] = waypoint, DSLPID            envs/BaseRLAviary.py:193-207 */
    GPD_ACT_VEL = 2,       /* a[0:4] = direction+speed, DSLPID     envs/BaseRLAviary.py:208-223.  A direction is zero (no
                              velocity asked) only if all three components are +-0; any other float32 direction, however small --
                              subnormal components, squares that underflow -- gives the unit vector of the float64 formula
                              (the components are rescaled by 2^100 before the norm when their squares sum below 2^-100;
                              an action whose squares sum to 2^-100 or more is computed as ever) */
    GPD_ACT_ONE_D_RPM = 3, /* rpm = HOVER_RPM*(1+0.05*a[0]) x4     envs/BaseRLAviary.py:224-225 */
    GPD_ACT_ONE_D_PID = 4, /* target = pos + 0.1*[0,0,a[0]], DSLPID envs/BaseRLAviary.py:226-235 */
    GPD_ACT_RAW_RPM = 5,   /* rpm = clip(a[0:4], 0, MAX_RPM)       envs/CtrlAviary.py:140 */
    GPD_ACT_DIRECT_RPM = 6 /* rpm = a[0:4] as is: the output of a user subclass's own
                              _preprocessAction (envs/BaseAviary.py:341,1051-1064) */
};

/* Aerodynamic add-on terms evaluated inside the explicit integrator
 * (envs/BaseAviary.py:354-367 dispatch; formulas :715-811), and the ground plane.
 *
 * GPD_PHYS_GROUND is NOT part of the reference's Physics.DYN (there the drone's pose is overwritten every step,
 * envs/BaseAviary.py:865-875, so the plane loaded at :479 never acts and a drone falls through z = 0).  It stands in
 * for what Bullet's solver does for Physics.PYB* with that plane: after every physics sub-step a drone whose collision
 * cylinder (URDF: COLLISION_H, COLLISION_Z_OFFSET) would sink below z = 0 is put back ON the plane
 * (z = params.ground_z), its downward velocity is removed (restitution 0) and it sticks laterally (vx = vy = 0); body
 * rates and attitude are left to the rigid-body equations.  "Would sink": z < ground_z, or z == ground_z with vz < 0 (a
 * resting drone whose downward velocity is too small to change its fp32 height is still in contact).  The Python classes
 * enable it for Physics.PYB* only.
 *
 * GPD_PHYS_DAMP is not part of the reference's Physics.DYN either.  It is the damping every Physics.PYB* run of the reference
 * carries without a line of the reference saying so: `p.loadURDF` (envs/BaseAviary.py:488-494) creates the drone as a Bullet
 * btMultiBody, whose default linear and angular damping is 0.04 (PyBullet's `changeDynamics` defaults; the reference never
 * changes them) and acts on the base as the forces  -M v d (1 + |v|)  and  -J w d (1 + |w|)  (Bullet 3.2.x,
 * src/BulletDynamics/Featherstone/btMultiBody.cpp, computeAccelerationsArticulatedBodyAlgorithmMultiDof, "adding damping
 * terms (only)", DAMPING_K1 = DAMPING_K2 = the coefficient; third-party source, not under the reference checkout: parity
 * unpinned).  Evaluated on the velocities at the start of the sub-step, like drag.  OPT-IN on the Python side (round 5): Physics.PYB*
 * enables GPD_PHYS_GROUND by default and GPD_PHYS_DAMP only with `pyb_like="damped"` / GPD_PYB_LIKE=damped, until
 * tests/test_pybullet_optional.py has pinned it on a box with PyBullet (`pyb_like=False` opts out of the plane too: the reference's
 * explicit integrator + the add-on models). */
enum { GPD_PHYS_GND = 1, GPD_PHYS_DRAG = 2, GPD_PHYS_DW = 4, GPD_PHYS_GROUND = 8, GPD_PHYS_DAMP = 16 };
#define GPD_BULLET_DAMPING 0.04f

/* Which task's reward / termination / truncation is evaluated in the step kernel */
enum {
    GPD_TASK_NONE = 0,       /* reward -1, never terminated/truncated (envs/CtrlAviary.py:144-190) */
    GPD_TASK_HOVER = 1,      /* envs/HoverAviary.py:68-117 */
    GPD_TASK_MULTIHOVER = 2  /* envs/MultiHoverAviary.py:75-130 */
};

enum {
    GPD_EINVAL = -1,   /* bad argument (NULL pointer, non-positive size, unknown enum) */
    GPD_ERANGE = -2,   /* size outside what the kernel supports (e.g. drones_per_env > 256) */
    GPD_ENOTSUP = -3   /* combination not supported (e.g. PID action on the RACE model) */
};

/*
 * Per-airframe constants.  Replaces the attributes BaseAviary.__init__ derives from the URDF
 * (envs/BaseAviary.py:97-128, _parseURDFParameters :985-1017) and the DSLPIDControl gains
 * (control/DSLPIDControl.py:37-60, control/BaseControl.py:35-39).  Passed BY VALUE in the
 * kernel argument segment, i.e. it lives in scalar registers: every field is wave-uniform.
 */
typedef struct GpdParams {
    int32_t drone_model;       /* GPD_MODEL_* */
    float M, inv_M;            /* mass [kg] and its reciprocal */
    float L;                   /* arm length [m] */
    float KF, KM;              /* thrust / torque coefficients */
    float GRAVITY;             /* G*M with G = 9.8            envs/BaseAviary.py:117 */
    float J[3], J_INV[3];      /* diagonal inertia and its inverse */
    float prop_x[4], prop_y[4];/* rotor offsets in the body frame (URDF prop links) */
    float gnd_eff_coeff, prop_radius, gnd_eff_h_clip;   /* envs/BaseAviary.py:128 */
    float drag_coeff[3];
    float dw_coeff[3];
    float hover_rpm, max_rpm;  /* envs/BaseAviary.py:118-119 */
    /* Rotor thrusts are carried as deviations from the hover thrust F_h = GRAVITY/4 (= KF*HOVER_RPM^2
     * exactly, envs/BaseAviary.py:118): g_i = KF*rpm_i^2 - F_h evaluated without cancellation, so that
     * "thrust minus weight" and the thrust differences that make the torques keep full fp32 relative
     * accuracy near hover (host-computed in float64): */
    float hover_thrust;        /* F_h = GRAVITY/4 */
    float hover_resid;         /* KF*float(HOVER_RPM)^2 - F_h: what rounding HOVER_RPM to fp32 leaves */
    float km_over_kf;          /* KM/KF */
    /* DSLPID (the RL aviaries always build CF2X controllers, envs/BaseRLAviary.py:75-76) */
    float pid_gravity, pid_kf; /* control/BaseControl.py:35-37 */
    float pid_inv_4kf;         /* 1/(4*pid_kf), host-computed in float64 */
    float p_for[3], i_for[3], d_for[3];
    float p_tor[3], i_tor[3], d_tor[3];
    float mixer[12];           /* row-major 4x3, control/DSLPIDControl.py:47-60 */
    float pwm2rpm_scale, inv_pwm2rpm_scale, pwm2rpm_const, min_pwm, max_pwm;
    float speed_limit;         /* ActionType.VEL, envs/BaseRLAviary.py:94-95 */
    float ground_z;            /* GPD_PHYS_GROUND: height of the base link when the collision cylinder rests on the
                                  plane, COLLISION_H/2 - COLLISION_Z_OFFSET (the 0.1 m the default INIT_XYZS adds on
                                  top of it, envs/BaseAviary.py:194-197) */
} GpdParams;

/*
 * Structure-of-arrays drone state; every row is a contiguous float[N] inside a [rows][ld]
 * block (ld >= N).  Replaces BaseAviary's pos/quat/vel/rpy_rates/last_clipped_action arrays and
 * the PyBullet state store (envs/BaseAviary.py:468-477, 509-519, 865-877) and the per-drone
 * DSLPIDControl members (control/DSLPIDControl.py:65-78).
 */
typedef struct GpdState {
    float* kin;            /* 13 x ld floats in FOUR PLANES (ABI 9; ABI <= 8: thirteen rows of ld floats):
                                P  float4[ld] at kin          (pos x, pos y, pos z, body rate x)
                                Q  float4[ld] at kin + 4 ld   (quat x, y, z, w)
                                V  float4[ld] at kin + 8 ld   (vel x, vel y, vel z, body rate y)
                                W  float [ld] at kin + 12 ld  body rate z
                              (body rates = the reference's rpy_rates, envs/BaseAviary.py:474).  A lane moves its drone with three
                              16-byte accesses and one 4-byte access per direction instead of thirteen 4-byte ones.
                              ALIGNMENT: kin must be 16-byte aligned (hipMalloc / torch allocations are; a sub-allocation at a
                              4-byte offset is not) -- every entry that moves the planes returns GPD_EINVAL otherwise */
    float* last_rpm;       /* [4][ld] last applied RPMs (last_clipped_action); NULL = not tracked
                              (required with GPD_PHYS_DRAG) */
    float* pid;            /* [9][ld]: integral_pos_e | last_rpy | integral_rpy_e; NULL unless a
                              PID action type is used */
    int32_t* step_counter; /* [num_envs] physics steps since reset (envs/BaseAviary.py:460,382) */
    int64_t ld;            /* row pitch in floats, 1 .. 2^32 - 1 (the kernels take it as a 32-bit argument; GPD_EINVAL beyond) */
    float* dw_force;       /* [ld] or NULL: body-z downwash force per drone computed OUTSIDE the step kernel
                              (gpd_downwash_global, for one aviary of more than 256 drones); used with
                              GPD_PHYS_DW when drones_per_env == 1, added in every sub-step of the call */
    /* Action history (the reference's action_buffer deque, envs/BaseRLAviary.py:65-67, 153-154, 187): a DOUBLE ring
     * of the raw actions, [2*hist_len][N][A] floats, slot-major -- every action is written to slots q and q + hist_len,
     * so that the hist_len most recent actions are always hist_len CONSECUTIVE slots, oldest first, starting at
     * ring_pos: the history tail of the observation row (:317-318) is a strided VIEW of the ring ([N][hist_len][A]
     * with strides A, N*A, 1), no copy.  A slot is one contiguous [N][A] block, the shape of an action input: the
     * push is a coalesced 16-byte store per lane.  Zero-filled at start (:153-154), never cleared by a reset
     * (SURVEY.md App. B.2).  gpd_step pushes its action itself when act_ring != NULL; after a gpd_rollout call
     * gpd_full_obs pushes the K actions of the call. */
    float* act_ring;       /* [2*hist_len][N][A] or NULL */
    int32_t* ring_pos;     /* [num_envs]: slot (0 .. hist_len-1) the NEXT action of the aviary goes to = where its oldest
                              one sits.  Kept on the device so that a captured hipGraph of steps replays correctly */
    int32_t hist_len;      /* H = ctrl_freq // 2 (envs/BaseRLAviary.py:65); 0 with act_ring == NULL */
    int32_t pad_;
    /* (ABI 8) Non-finite guard, optional: every call that writes the state back (gpd_step, gpd_rollout*, gpd_rollout_policy,
     * gpd_swarm_step) also stores one byte per drone -- 1 if any of the drone's 13 kinematic floats is NaN or +-inf in the
     * state it leaves behind, else 0.  The reference has no such check (a NaN action silently poisons `pos` / `quat` for the rest
     * of the episode, envs/BaseAviary.py:831-877); a NaN position also never trips a truncation bound
     * (every comparison is false), so without the flag a poisoned aviary runs on until the episode clock ends it.  (Deviation for
     * garbage input, DSLPID action types only: a NaN set-point is absorbed by the controller's clips -- the hardware min/max return
     * the bound where numpy's clip propagates the NaN -- so the drone sees one step of saturated commands and stays finite.)  (Two more
     * states that heal, both by the model's own rules: under GPD_PHYS_GROUND a height of -inf is below the plane, so the next sub-step
     * puts the drone on it and it ends finite; and a NaN in the quaternion reads pitch = -pi/2 -- the clamp in front of the arcsine
     * returns its bound -- which trips tilt_bound: a task with that bound truncates the aviary in the same step, and auto_reset then
     * resets it.  Without either the state stays non-finite and the byte stays 1.)  Costs
     * thirteen adds and a compare per drone and launch, outside the step loop.  The byte describes the state the call LEAVES BEHIND: an
     * aviary that went non-finite inside a K-step launch and was reset by its episode clock in the same launch (auto_reset) ends finite
     * and reads 0 -- a caller that must see every event checks between shorter launches. */
    uint8_t* bad;          /* [N] or NULL */
} GpdState;

/* Per-call configuration of gpd_step */
typedef struct GpdStepCfg {
    int32_t num_envs;        /* E */
    int32_t drones_per_env;  /* D, 1..256 */
    int32_t act_type;        /* GPD_ACT_* */
    int32_t substeps;        /* PYB_STEPS_PER_CTRL = pyb_freq/ctrl_freq  envs/BaseAviary.py:81 */
    uint32_t physics_flags;  /* GPD_PHYS_* mask */
    float pyb_dt;            /* PYB_TIMESTEP   envs/BaseAviary.py:83 */
    float ctrl_dt;           /* CTRL_TIMESTEP  envs/BaseAviary.py:82 */
    float inv_ctrl_dt;       /* CTRL_FREQ as a float (exact), multiplies where the reference divides by dt */
    int32_t lanes_per_wave;  /* 16, 32 or 64 drones per 64-lane wavefront when drones_per_env == 1 (0 = 64):
                                fewer active lanes = more wavefronts per SIMD = shorter critical path when
                                the batch is too small to fill the chip (latency-bound regime) */
    int32_t task;            /* GPD_TASK_* */
    float xy_bound, z_bound, tilt_bound;  /* truncation box  envs/HoverAviary.py:110-111 */
    float term_dist;         /* 1e-4            envs/HoverAviary.py:93 */
    int32_t trunc_counter;   /* truncated iff step_counter > trunc_counter, i.e.
                                step_counter/PYB_FREQ > EPISODE_LEN_SEC  envs/HoverAviary.py:114 */
    int32_t target_per_env;  /* 0: target_pos is [D][3] shared by all envs; 1: [E*D][3] */
    int32_t init_per_env;    /* 0: init_pose is [D][7] shared by all envs; 1: [E*D][7] */
    int32_t auto_reset;      /* 1: envs that end (terminated|truncated) are reset in the same call,
                                the SB3 DummyVecEnv convention (examples/learn.py:54-58) */
} GpdStepCfg;

/* ABI version of the loaded library (== GPD_ABI_VERSION of the header it was built from). */
int gpd_abi_version(void);

/* Description of the last error on the calling thread ("" if none). */
const char* gpd_last_error(void);

/* sizeof(GpdParams), sizeof(GpdState), sizeof(GpdStepCfg): lets a binding verify its struct
 * mirrors before the first call. */
void gpd_struct_sizes(int32_t out[3]);

/*
 * One env.step() for E aviaries of D drones.  Replaces BaseAviary.step's hot body
 * (envs/BaseAviary.py:341-382): _preprocessAction (envs/BaseRLAviary.py:160-239, incl.
 * DSLPIDControl.computeControl, control/DSLPIDControl.py:82-259), `substeps` x { _dynamics +
 * _integrateQ (:815-892) with the _groundEffect/_drag/_downwash terms (:715-811) },
 * _updateAndStoreKinematicInformation (:509-519), the kinematic part of _computeObs
 * (envs/BaseRLAviary.py:307-315), _computeReward/_computeTerminated/_computeTruncated
 * (envs/HoverAviary.py:68-117, envs/MultiHoverAviary.py:75-130) and the step-counter update.
 *
 *   action      [E*D][A] row-major, A = 4 (RPM, VEL, RAW_RPM), 3 (PID), 1 (ONE_D_*)
 *   target_pos  [D][3] or [E*D][3]: TARGET_POS of the task (ignored for GPD_TASK_NONE, may be NULL)
 *   init_pose   [D][7] or [E*D][7]: INIT_XYZS xyz + quaternion of INIT_RPYS; used by auto_reset
 *               only (may be NULL when auto_reset == 0)
 *   obs12       [E*D][12] out: pos | rpy | vel | ang_v   (envs/BaseRLAviary.py:314); with
 *               auto_reset it holds the post-reset observation of the envs that ended
 *   reward      [E] out
 *   terminated  [E] out (0/1), truncated [E] out (0/1)
 *   term_obs12  [E*D][12] out or NULL: with auto_reset, rows of envs that ended receive the last
 *               observation of the finished episode (SB3's info["terminal_observation"]); other
 *               rows are left untouched
 */
int gpd_step(const GpdParams* params, const GpdState* state, const GpdStepCfg* cfg,
             const float* action, const float* target_pos, const float* init_pose,
             float* obs12, float* reward, uint8_t* terminated, uint8_t* truncated,
             float* term_obs12, void* stream);

/*
 * gpd_step, then a wait for it on `stream`: returns when the step's results are where the kernel wrote them (and everything queued
 * on the stream before it has completed).  How it waits is the library's business: a launch whose drones fit one wavefront (up to
 * 64 drones) ends with a release store of a sequence number into a page-locked word the calling thread spins on (7.6 us for an
 * empty kernel on MI355X where launch + hipStreamSynchronize takes 12.4); every other shape, and a word that stays silent for
 * 2 ms, waits with hipStreamSynchronize.
 * The one call behind the reference-shaped single aviaries (`BaseAviary.step`, envs/BaseAviary.py:259-383 of the reference: its
 * step() returns numpy values, so every step ends in a host read): their state, action row and outputs live in page-locked HOST
 * memory mapped into the device's address space (hipHostMalloc -- every pointer of this ABI may be such a host pointer), the
 * kernel reads and writes them over the link, and the host reads the results in place -- no copy engine, no second launch, one
 * library call per step.  Same arguments and error codes as gpd_step; a failed wait returns the positive hipError_t.
 */
int gpd_step_sync(const GpdParams* params, const GpdState* state, const GpdStepCfg* cfg,
                  const float* action, const float* target_pos, const float* init_pose,
                  float* obs12, float* reward, uint8_t* terminated, uint8_t* truncated,
                  float* term_obs12, void* stream);

/*
 * K consecutive env.step() calls in ONE launch.  Replaces the caller's stepping loop around
 * BaseAviary.step when the actions of the K steps are known up front: open-loop RPM sequences, and
 * closed-loop DSLPID tracking of a precomputed waypoint list -- the loops of examples/pid.py:132-167
 * and examples/downwash.py:93-113 (`for i in range(...): obs, ... = env.step(action)` with
 * `TARGET_POS[wp_counters[j]]` as the controller's target) -- or a fixed action
 * (action_step_stride == 0, e.g. ActionType.PID holding one waypoint, examples/learn.py:157-192 with a
 * constant policy output).  The drone state is read once, kept in registers for all K steps and
 * written once; per step only the action row is read and the observation row / reward / flags are
 * written, so the per-step HBM traffic drops from ~182 B to ~70 B per drone and the ~2 us
 * launch-to-launch latency is paid once per K steps instead of once per step.  Bitwise identical to
 * K calls of gpd_step (same instructions in the same order).
 *
 *   num_steps          K >= 1
 *   actions            step t reads [E*D][A] at actions + t*action_step_stride (floats);
 *                      action_step_stride = 0 repeats one action block for all K steps
 *   obs12              step t writes [E*D][12] at obs12 + t*obs_step_stride (floats); stride 0 keeps
 *                      only the last step's observation (each step overwrites the block)
 *   reward/terminated/truncated
 *                      step t writes [E] at base + t*env_step_stride (elements); stride 0 keeps only
 *                      the last step's values
 *   term_obs12         NULL, or laid out like obs12 (same stride): with auto_reset, the rows of step t
 *                      of the envs that ended at step t receive the last observation of the episode
 *   everything else as in gpd_step.
 */
int gpd_rollout(const GpdParams* params, const GpdState* state, const GpdStepCfg* cfg,
                int32_t num_steps, const float* actions, int64_t action_step_stride,
                const float* target_pos, const float* init_pose,
                float* obs12, int64_t obs_step_stride,
                float* reward, uint8_t* terminated, uint8_t* truncated, int64_t env_step_stride,
                float* term_obs12, void* stream);

/*
 * gpd_rollout that ALSO pushes every step's raw action into the action ring of `state` (act_ring / ring_pos / hist_len), the
 * way gpd_step does: for a consumer that keeps the history as the zero-copy view (envs/BaseRLAviary.py:65-67, 153-154, 187) and
 * needs no materialised rows -- the K actions never take the detour through a second kernel (gpd_full_obs with obs_full =
 * NULL does the same after a plain gpd_rollout, re-reading them: 1.72 vs 1.29 us per step at 65 536 drones).  No terminal
 * observations; aviaries of up to 64 drones (GPD_ENOTSUP otherwise: use gpd_rollout + gpd_full_obs).
 */
int gpd_rollout_history(const GpdParams* params, const GpdState* state, const GpdStepCfg* cfg, int32_t num_steps,
                        const float* actions, int64_t action_step_stride, const float* target_pos, const float* init_pose,
                        float* obs12, int64_t obs_step_stride, float* reward, uint8_t* terminated, uint8_t* truncated,
                        int64_t env_step_stride, void* stream);

/*
 * Domain randomisation: a plant of its own for every drone.  GpdParams is one airframe for the whole launch; the plant path gives
 * each drone NINE SCALE FACTORS relative to that nominal airframe, [GPD_NUM_SCALES][ld] floats (drone n at scales + s*ld + n):
 */
enum {
    GPD_SCALE_MASS = 0,    /* M                          */
    GPD_SCALE_IXX = 1,     /* J[0]                       */
    GPD_SCALE_IYY = 2,     /* J[1]                       */
    GPD_SCALE_IZZ = 3,     /* J[2]                       */
    GPD_SCALE_KF = 4,      /* KF                         */
    GPD_SCALE_KM = 5,      /* KM                         */
    GPD_SCALE_DRAG_XY = 6, /* DRAG_COEFF[0], DRAG_COEFF[1] */
    GPD_SCALE_DRAG_Z = 7,  /* DRAG_COEFF[2]              */
    GPD_SCALE_GND_EFF = 8, /* GND_EFF_COEFF              */
    GPD_NUM_SCALES = 9
};
/*
 * Everything derived from them follows (GRAVITY = G*M, inv_M, J_INV, KM/KF, the hover-thrust terms).  THE PLANT CHANGES, WHAT THE
 * AGENT AND THE CONTROLLER KNOW DOES NOT: HOVER_RPM of the action mapping, the MAX_RPM clip, DSLPID's model and gains (pid_*), the
 * speed limit, arm length and rotor positions, the downwash coefficients, gnd_eff_h_clip and ground_z stay those of GpdParams.  A
 * drone with mass 1.2 that receives action 0 sinks.  Scales are finite and > 0; a drone whose scales are all 1.0 flies the nominal
 * airframe bit for bit.
 *
 * The DERIVED PLANT ROWS are what the kernels read: [GPD_PLANT_ROWS][ld] floats, the state's SoA convention (drone n at
 * rows + r*ld + n, indexed like GpdState.kin), 16-byte aligned.  Row r replaces, in the plant, the GpdParams field named: */
enum {
    GPD_PLANT_M = 0,            /* M                 (Bullet damping)                 M_n * s_mass                        */
    GPD_PLANT_INV_M = 1,        /* inv_M                                              inv_M_n / s_mass                    */
    GPD_PLANT_KF = 2,           /* KF                (raw-RPM and DSLPID thrust)      KF_n * s_kf                         */
    GPD_PLANT_GRAVITY = 3,      /* GRAVITY                                            GRAVITY_n * s_mass                  */
    GPD_PLANT_J = 4,            /* J[0..2]           rows 4, 5, 6                     J_n[k] * s_ixx / s_iyy / s_izz      */
    GPD_PLANT_J_INV = 7,        /* J_INV[0..2]       rows 7, 8, 9                     J_INV_n[k] / s_ixx / s_iyy / s_izz  */
    GPD_PLANT_KM_OVER_KF = 10,  /* km_over_kf                                         km_over_kf_n * s_km / s_kf          */
    GPD_PLANT_GND_EFF = 11,     /* gnd_eff_coeff                                      gnd_eff_coeff_n * s_gnd_eff         */
    GPD_PLANT_DRAG = 12,        /* drag_coeff[0..2]  rows 12, 13, 14                  drag_n[k] * s_drag_xy / s_drag_z    */
    GPD_PLANT_HOVER_THRUST = 15,/* hover_thrust      F_h = GRAVITY/4 of the drone     hover_thrust_n * s_mass             */
    GPD_PLANT_HOVER_RESID = 16, /* hover_resid       KF*float(HOVER_RPM_n)^2 - F_h    hover_resid_n*s_kf + (s_kf - s_mass)*hover_thrust_n */
    GPD_PLANT_NORM_THRUST = 17, /* (new) T = KF*HOVER_RPM_n^2: thrust of the normalised action 0   hover_thrust_n * s_kf      */
    GPD_PLANT_NORM_GAP = 18,    /* (new) F_h - T: what the normalised action types' deviation subtracts   (s_mass - s_kf)*hover_thrust_n */
    GPD_PLANT_ROWS = 19         /* 76 bytes per drone */
};
/*
 * (The rows are derived from the nominal struct's fp32 fields in float64 and rounded once, so that a row of 1.0 scales reproduces
 * them exactly: every formula above is the nominal field times or over 1.0, plus 0.)
 *
 * gpd_plant_derive: rows <- derive(nominal, scales) for the drones of the aviaries whose env_mask byte is non-zero (env_mask == NULL:
 * all num_envs * drones_per_env drones; drone n belongs to aviary n / drones_per_env, as in gpd_reset).  Rows of other drones are
 * left untouched.  No check of the scales' values on the device (the caller validates them once).
 *
 * gpd_rollout_plant: gpd_rollout with the plant rows (pitch state.ld, like the state) -- one entry for step() (num_steps = 1: the
 * single-step kernel, as gpd_rollout routes a one-step rollout) and rollout().  Every other argument as in gpd_rollout; the action
 * ring of `state` is ignored (gpd_full_obs pushes after the call).  Served by generic kernels of their own (the PLANT = true
 * instantiations of gpd_step_kernel, gpd_rollout1_kernel and gpd_rollout_kernel) for every shape gpd_rollout serves, except state.dw_force (one aviary of more than 256 drones,
 * gpd_downwash_global): GPD_ENOTSUP.
 * Both entries validate before any device work: NULL pointers, ld < num_envs * drones_per_env, rows not 16-byte aligned.
 */
int gpd_plant_derive(const GpdParams* nominal, const float* scales, const uint8_t* env_mask, int32_t num_envs,
                     int32_t drones_per_env, int64_t ld, float* rows, void* stream);
int gpd_rollout_plant(const GpdParams* params, const GpdState* state, const GpdStepCfg* cfg, int32_t num_steps,
                      const float* actions, int64_t action_step_stride, const float* target_pos, const float* init_pose,
                      float* obs12, int64_t obs_step_stride, float* reward, uint8_t* terminated, uint8_t* truncated,
                      int64_t env_step_stride, float* term_obs12, const float* plant_rows, void* stream);

/*
 * A deterministic MLP policy evaluated INSIDE the rollout kernel: the actor of Stable-Baselines3's default `MlpPolicy`
 * (features -> Linear(in_dim, 64) -> tanh -> Linear(64, 64) -> tanh -> Linear(64, act_dim), `model.predict(obs,
 * deterministic=True)` incl. its clip to the action space [-1, 1]) -- what examples/learn.py:157-192 evaluates between two
 * env.step() calls.  Weights are float32 device arrays in torch's Linear layout (weight [out][in] row-major, bias [out]).
 *   in_dim = 12                       the policy sees the kinematic observation only
 *   in_dim = 12 + hist_len*act_dim    the policy sees the reference's full row (BaseRLAviary._computeObs): kinematics, then the
 *                                     hist_len most recent actions, oldest first (state->act_ring must be set)
 * activation: 0 = tanh (SB3's default), 1 = ReLU.
 */
typedef struct GpdPolicy {
    const float* w1; const float* b1;   /* [64][in_dim], [64] */
    const float* w2; const float* b2;   /* [64][64], [64] */
    const float* w3; const float* b3;   /* [act_dim][64], [act_dim] */
    int32_t in_dim;
    int32_t hidden;                     /* 64 */
    int32_t activation;                 /* 0 tanh, 1 relu */
    int32_t pad_;
} GpdPolicy;

/*
 * K consecutive env.step() calls in ONE launch with the policy IN the loop.  Replaces the evaluation / sampling loop of
 * examples/learn.py:157-192 (`action, _ = model.predict(obs, deterministic=True); obs, reward, terminated, truncated, info =
 * env.step(action)`), for single-drone aviaries (HoverAviary) and all five ActionTypes (for PID / VEL / ONE_D_PID the policy's
 * output is the set-point of the embedded DSLPID controller, which runs inside the same step):
 *     a_t = clip(W3 act(W2 act(W1 o_t + b1) + b2) + b3, -1, 1);   o_{t+1}, r_t, ... = step(a_t)
 * where o_t is the latest observation row -- of the reset pose when the aviary was reset in step t-1 (same-step auto-reset, the
 * history tail survives resets like the reference's action buffer).  The drone state stays in registers for all K steps like in
 * gpd_rollout; the two 64-unit layers run on the matrix cores: the 64 drones of a wavefront are the columns of
 * v_mfma_f32_32x32x16_bf16 tiles, every operand split into bf16 hi + lo parts (three products per tile: hi*hi + hi*lo + lo*hi,
 * fp32 accumulate), which keeps ~16 mantissa bits of the float32 weights and observations (actions agree with a float64
 * evaluation to ~1e-5); a layer's output tile is the next layer's B operand without leaving registers.
 *
 *   obs12_in     [E][12] the latest observation rows (the obs12 output of the previous step / reset / rollout)
 *   actions_out  [K][E][A] out or NULL: the actions the policy chose, step t at actions_out + t*E*A
 *   obs12 / reward / terminated / truncated and the strides: as in gpd_rollout
 *   noise, action_std, mean_out   training rollouts (all NULL: the deterministic policy above).  The collection loop of
 *                Stable-Baselines3's PPO (`model.learn()`, examples/learn.py:61-95: DiagGaussianDistribution with a
 *                state-independent log_std, actions clipped to the Box before env.step):
 *                    a_t = clip(mean_t + action_std[k] * noise[t][e][k], -1, 1)
 *                noise [K][E][A]: standard-normal draws of the caller (device memory); action_std [A]: exp(log_std), HOST
 *                memory; mean_out [K][E][A] out or NULL: the unclipped means.  actions_out and the action ring receive the
 *                clipped actions (what the environment saw); the log-probability of the unclipped sample is a function of
 *                noise and action_std alone.  ActionType.RPM and ONE_D_RPM.
 * With in_dim > 12 the action ring of `state` is read at the start, and EVERY step pushes its (clipped) action into both halves
 * of the ring and advances ring_pos by one (mod hist_len), exactly as gpd_step does: after the call the ring and ring_pos are what
 * num_steps gpd_step calls with the same actions would have left (history() / gpd_hist_rows / a following gpd_step continue
 * seamlessly).
 *   term_obs12   (ABI 8) NULL, or laid out like obs12 (same stride): with auto_reset, the rows of step t of the aviaries that ended
 *                at step t receive the last observation of the finished episode -- SB3's info["terminal_observation"], which its
 *                PPO bootstraps time-outs from (examples/learn.py:61-95 through `model.learn()`); other rows are left untouched.
 * GPD_ENOTSUP: drones_per_env > 1, hidden != 64, in_dim not one of the two forms, or a history longer than 17 actions of 4 or
 * 3 floats / 20 actions of 1 float (the reference's 30 Hz control: 15).
 */
int gpd_rollout_policy(const GpdParams* params, const GpdState* state, const GpdStepCfg* cfg, const GpdPolicy* policy,
                       int32_t num_steps, const float* obs12_in, const float* target_pos, const float* init_pose,
                       float* actions_out, float* obs12, int64_t obs_step_stride, float* reward, uint8_t* terminated,
                       uint8_t* truncated, int64_t env_step_stride, const float* noise, const float* action_std, float* mean_out,
                       float* term_obs12, void* stream);

/*
 * Full KIN observation rows with the action-history tail.  Replaces the row assembly of BaseRLAviary._computeObs
 * (envs/BaseRLAviary.py:307-320) on top of the action ring of GpdState (which replaces the deque, :65-67, 153-154, 187):
 *     row = [ pos | rpy | vel | ang_v | a(t-H+1) ... a(t) ]      H = ctrl_freq // 2, oldest action first
 * The rows are MATERIALISED only on request -- at 240 Hz control a row is 12 + 120*4 floats, ten times the bytes of the
 * whole physics step; a consumer that can take (obs12, history view) separately never needs them.
 *
 * gpd_hist_rows: the current rows, after a gpd_step call (which pushed its action into the ring itself):
 *   state       act_ring / ring_pos / hist_len are read (ring_pos of aviary n / drones_per_env)
 *   obs12       [n_drones][12] of the latest step
 *   obs_full    [n_drones][12 + hist_len*act_dim] out
 *
 * gpd_full_obs: the rows of the num_steps steps of a gpd_rollout call (call it after the rollout, same stream), built
 * from the ring as the rollout found it plus the call's own action blocks; then the K actions are pushed into the ring
 * and ring_pos advances by num_steps (mod hist_len).
 *   obs12         the rollout's observation blocks, step t at obs12 + t*obs_step_stride
 *   actions       the rollout's action blocks,      step t at actions + t*action_step_stride (0: held action)
 *   obs_full      [num_steps][n_drones][12 + hist_len*act_dim] out, step t at obs_full + t*full_step_stride;
 *                 NULL: only update the ring
 */
int gpd_hist_rows(const GpdState* state, int32_t n_drones, int32_t drones_per_env, int32_t act_dim, const float* obs12,
                  float* obs_full, void* stream);
int gpd_full_obs(const GpdState* state, int32_t num_steps, int32_t n_drones, int32_t drones_per_env, int32_t act_dim,
                 const float* obs12, int64_t obs_step_stride, const float* actions, int64_t action_step_stride,
                 float* obs_full, int64_t full_step_stride, void* stream);

/*
 * Downwash forces inside ONE aviary of n drones, any n (the step kernel itself handles aviaries of up to 256
 * drones).  Replaces the O(n^2) Python loop of BaseAviary._downwash (envs/BaseAviary.py:785-811) over all pairs
 * with  dz = z_j - z_i > 0  and  dxy < 10 m:
 *     F_i = - sum_j  DW1 * (PROP_RADIUS / (4 dz))^2 * exp(-0.5 * (dxy / (DW2*dz + DW3))^2)        (body z of drone i)
 * by binning the drones into a uniform 2-D grid of `cell` >= 10 m squares (counting sort by cell) and searching
 * the 3x3 neighbourhood of each drone's cell.  The grid is periodic: a drone outside the box the grid was laid over
 * lands in the cell its coordinates wrap to (still exact: every candidate pair is distance-tested, aliased far-apart
 * drones are rejected; the swarm may spread without piling up in border cells).  The per-drone sum is accumulated
 * in 64-bit fixed point (2^-30 N), so the result does not depend on the order the sort leaves the neighbours in; a pair
 * whose exponent 0.5 (dxy / (DW2*dz + DW3))^2 reaches 40 is dropped (it is below e^-40 = 4.3e-18 of its own amplitude).
 *
 *   kin, ld       the state block of gpd_step (plane P = positions is read: float4 n at kin + 4 n)
 *   cell, x0, y0, nx, ny   grid: cell size [m] (>= 10), lower-left corner, cells per side (nx, ny >= 3)
 *   z0, zbin, nz  every cell is split into nz height bins of zbin metres starting at z0 (bin 0 also holds everything below z0,
 *                 bin nz-1 everything above; nz = 1: no bins, z0/zbin ignored); nx*ny*nz <= 65536.  The sort key is
 *                 cell*nz + bin, so inside a cell the drones are ordered by height bin.  Ordering only: any (z0, zbin, nz)
 *                 gives the same forces bit for bit (the force kernel of ABI 4's first builds pruned by bin; the present
 *                 one does not, nz = 1 is the sensible choice).
 *   visit_order   [n] int32 permutation of 0..n-1 or NULL (= 0, 1, 2 ...): the order the sort visits the drones in.
 *                 Any permutation gives the same forces bit for bit; handing in the `order` buffer the PREVIOUS call
 *                 filled (two buffers, ping-pong: it must not alias `order`) makes neighbouring lanes share a cell, and
 *                 the sort then issues one atomic per run of equal cells instead of one per drone.
 *   cell_count    [2 (nx*ny*nz + 1)] int32 (per-key counts | per-key cursors of the sort): ZERO before the first call; every
 *                 call leaves it zeroed again (the last kernel clears it: no memset per call)
 *   cell_start    [nx*ny*nz + 1] int32 scratch
 *   order         [n] int32 out (drone index of sorted slot: a permutation of 0..n-1)
 *   sorted_xyzc   [n][4] float scratch (x, y, z, sort key as int bits), sorted by key
 *   dw_out        [n] out: the force of drone i at dw_out[i]  (pass it to gpd_step as state.dw_force)
 *   vec_state, vec_obs12, vec_out   optional (vec_out NULL: none): the sort's first pass also writes the [n][20] state vectors
 *                 of gpd_state_vectors(vec_state, vec_obs12, vec_out, n) -- a caller that computes the forces for the NEXT
 *                 sub-step right after a gpd_step needs both, and saves a launch
 * Call it once per physics sub-step, before the gpd_step launch of that sub-step (positions are the snapshot every
 * drone sees, envs/BaseAviary.py:346-347).
 */
int gpd_downwash_global(const GpdParams* params, const float* kin, int64_t ld, int32_t n, float cell, float x0,
                        float y0, int32_t nx, int32_t ny, float z0, float zbin, int32_t nz, const int32_t* visit_order,
                        int32_t* cell_count, int32_t* cell_start, int32_t* order, float* sorted_xyzc, float* dw_out,
                        const GpdState* vec_state, const float* vec_obs12, float* vec_out, void* stream);

/*
 * ONE aviary of any size, stepped by one or several ranks (GPUs): the persistent form of gpd_downwash_global.
 *
 * What changes against calling gpd_downwash_global before every gpd_step (count + scan/scatter + force + step = four
 * dependent launches per physics sub-step):
 *   - the physics sub-step kernel (gpd_swarm_step: gpd_step's arithmetic for single-drone lanes) ALSO writes the drone's new
 *     position into a packed [rows][4] array, tracks how far it has moved since the drones were last binned, and (on request)
 *     writes the drone's 20-float state vector: no separate pass over the drones after a step;
 *   - the counting sort (gpd_swarm_bin) runs every few sub-steps only.  Between two binnings the force kernel
 *     (gpd_swarm_forces) works on the STALE cell order but on CURRENT positions (slot -> row -> pos4), and widens its search
 *     from 3x3 cells to (2R+1)x(2R+1), R = ceil((10 m + 2 dmax) / cell), dmax = the largest displacement of any
 *     drone since the binning: two drones within 10 m of each other now were within 10 m + 2 dmax then, i.e. at most R cells
 *     apart.  With cell = 10 m + a skin, R stays 1 until some drone has moved half the skin; whatever the drones do, every
 *     pair the reference would sum (dz > 0, dxy < 10 m; envs/BaseAviary.py:785-811) is evaluated, on current positions, in
 *     order-independent 64-bit fixed point: the forces are the ones gpd_downwash_global returns, bit for bit.  (R beyond 3,
 *     or beyond the grid: the group sweeps every drone.)  A sub-step is then TWO launches: gpd_swarm_step, gpd_swarm_forces;
 *   - several ranks share one world: rank r owns the rows [r*slab, (r+1)*slab) -- its own_count drones, then rows without a
 *     drone (non-finite x), the LAST meta_rows rows of the slab being the rank's meta rows (NaN, sum dx, sum dy, w): workgroup b
 *     of gpd_swarm_step stores the largest squared displacement of its 256 drones in the w of meta row b (and their summed
 *     lateral displacements in y, z) -- plain stores, the force kernel takes the maximum.  After
 *     gpd_swarm_step every rank all-gathers its slab IN PLACE (gpd_allgather_obs(comm, pos4 + rank*slab*4, pos4, slab*4):
 *     16 bytes per drone, the one collective per sub-step), bins ALL rows when a binning is due (every rank the same
 *     sub-steps), and evaluates the forces of ITS drones only (workgroups of the sorted array without a drone of the rank
 *     exit at once).  Sums are integers: a world stepped by 1, 2 or 8 ranks follows the same trajectory bit for bit.
 *
 * The force of own drone i lands in dw_force[i]: pass it to gpd_swarm_step as state.dw_force (GPD_PHYS_DW).
 */
typedef struct GpdSwarm {
    int32_t n_rows;        /* rows of pos4 = world_size * slab */
    int32_t slab;          /* rows per rank (>= own_count + meta_rows: the last meta_rows are its meta rows) */
    int32_t world_size, rank;
    int32_t own_count;     /* drones of this rank: rows rank*slab .. rank*slab + own_count - 1 */
    int32_t nx, ny, nz;    /* grid: cells per side (>= 3 each), height bins per cell (1: none); nx*ny*nz <= 65536 */
    float cell, x0, y0;    /* cell size [m] (>= 10), lower-left corner of the (periodic) grid */
    float z0, zbin;        /* height bins as in gpd_downwash_global (ordering only) */
    int32_t meta_rows;     /* >= ceil(max own_count / 256), the same on every rank: one row per workgroup of gpd_swarm_step */
    float* pos4;           /* [n_rows][4] x, y, z, - of every row (meta rows: w = a partial dmax^2) */
    float* bin_pos;        /* [n_rows][4] x, y, z, - of every row at the last binning */
    int32_t* cell_count;   /* [2 (nx*ny*nz + 1)] counts | cursors: ZERO before the first gpd_swarm_bin.  gpd_swarm_bin leaves the counts
                              and cursors of its sort in it; the gpd_swarm_forces call that must follow every binning (build_lists
                              or not) clears them again -- no memset per call.  Two gpd_swarm_bin calls WITHOUT a gpd_swarm_forces
                              in between (re-pack + re-bin) need the caller to zero the array itself: the second sort would
                              otherwise start from the first one's counts and scatter out of bounds */
    int32_t* cell_start;   /* [nx*ny*nz + 1] */
    int32_t* order;        /* [n_rows] sorted slot -> row, written by gpd_swarm_bin, read by gpd_swarm_forces: ONE buffer, always that
                              of the latest binning (a captured hipGraph of sub-steps replays correctly whatever ran in between) */
    const int32_t* visit;  /* [n_rows] or NULL: the order gpd_swarm_bin visits the rows in -- any permutation gives the same forces;
                              the previous binning's order makes neighbouring lanes share a cell (one atomic per run of equal
                              cells).  Must alias neither `order` nor `visit_out` ... */
    int32_t* visit_out;    /* ... [n_rows] or NULL: gpd_swarm_bin writes a second copy of `order` here -- hand it in as `visit` next
                              time and the old `visit` buffer as `visit_out` (ping-pong; which of the two holds the newer copy
                              does not matter for correctness) */
    int32_t* slot_key;     /* [n_rows] sort key (cell*nz + bin) of every sorted slot */
    float* dw_force;       /* [>= own_count] out: body-z downwash force of own drone i (envs/BaseAviary.py:805-811) */
    /* world_size == 1 only (both NULL otherwise): the positions ALSO by sorted slot, kept current by gpd_swarm_step, so that the
     * force kernel reads its candidates as contiguous stretches instead of through order[] (a rank that holds the whole world
     * needs no exchange in row order) */
    int32_t* slot_of;      /* [n_rows] row -> sorted slot (-1: no finite position), written by gpd_swarm_bin */
    float* pos_sorted;     /* [n_rows][4] */
    /* Wake lists (optional: pair_list NULL = none).  The force launch right after a binning (build_lists != 0) keeps every pair
     * that could pass the model's tests once both drones have moved up to list_delta, and writes the pairs it evaluates to
     * pair_list; the launches until the next binning read them back instead of sweeping all candidates -- as long as no drone is
     * further than list_delta from where it was binned (otherwise they sweep as if there were no lists: still exact).
     * list_delta: just under (cell - 10 m) / 2, e.g. 0.49 (cell - 10). */
    uint32_t* pair_list;   /* [ceil(n_rows / 64)][4][list_cap * 64]: (ABI 8) 32-bit entries -- 6 bits drone of the group, 26 bits the
                              candidate's index in the array its position is read from (sorted slot / row of pos4): a replay launch
                              gathers the candidates' current positions directly, no cell table, no staged tile */
    uint16_t* pair_nb;     /* [ceil(n_rows / 64)][4][16]: [0] = batches the wavefront recorded */
    int32_t* list_ok;      /* [ceil(n_rows / 64)] */
    int32_t list_cap;      /* batches of 64 pairs per wavefront (a group of 64 drones has four), 4 .. 65535; a group that needs more sweeps */
    float list_delta;
    /* "Displacement" above is measured relative to the swarm's COMMON lateral drift since the binning (a translation all drones
     * share changes no pair: a swarm in transit keeps R = 1 and its wake lists).  gpd_swarm_forces computes the drift -- the mean
     * lateral displacement of all drones, from per-workgroup sums in the meta rows (y, z) -- for the next gpd_swarm_step. */
    float* drift;          /* [4] device floats, zero before the first call: [0..1] the drift (gpd_swarm_bin zeroes them), [2] the
                              margin of the wake lists of the current binning (gpd_swarm_bin sets it, below), [3] reserved */
    int32_t total_drones;  /* drones of the whole world (all ranks) */
    int32_t list_adapt;    /* (ABI 7) 0: the lists' margin is list_delta.  1: gpd_swarm_bin chooses it for each binning from the
                              displacement the interval that ends there has seen -- min(list_delta, max(1 cm, 3 dmax)): a swarm
                              that hovers lists hardly more pairs than the exact tests keep (at cell = 10.5 m the full margin
                              lists 40 % more); one that moves further than expected sweeps until the next binning.  Exact
                              either way. */
} GpdSwarm;

/* One physics sub-step of the rank's own_count drones (state / cfg as for gpd_step: drones_per_env = 1, num_envs = own_count,
 * substeps = 1, task NONE, no auto-reset; act_type RPM, RAW_RPM or DIRECT_RPM; state.dw_force = swarm.dw_force with
 * GPD_PHYS_DW), plus: pos4 rows of the rank, the rank's dmax^2, and -- vec_out != NULL -- the [own_count][20] state vectors
 * of gpd_state_vectors.  Replaces the body of BaseAviary.step's sub-step loop for one world (envs/BaseAviary.py:346-372).
 * When world_size * meta_rows > 1024 the call also leaves the rank's largest dmax^2 in the w of the rank's FIRST meta row (a second,
 * one-workgroup launch): gpd_swarm_forces then reads one value per rank instead of every meta row. */
/* sizeof(GpdSwarm), for a binding to verify its mirror (gpd_struct_sizes covers the three structs of ABI 1). */
int gpd_sizeof_swarm(void);

int gpd_swarm_step(const GpdParams* params, const GpdState* state, const GpdStepCfg* cfg, const GpdSwarm* swarm,
                   const float* action, float* obs12, float* vec_out, void* stream);
/* After a reset / any outside change of the state: pos4 rows of the rank (and its drone-less rows and meta row) from
 * state.kin, dmax^2 = 0, optionally the state vectors.  Follow it with the all-gather, gpd_swarm_bin and gpd_swarm_forces. */
int gpd_swarm_pack(const GpdState* state, const GpdSwarm* swarm, const float* obs12, float* vec_out, void* stream);
/* Counting sort of ALL rows by grid cell from pos4 (rows with a non-finite position take no part): order, slot_key,
 * cell_start, bin_pos (cell_count must be zero on entry: see GpdSwarm -- every binning is followed by gpd_swarm_forces); every rank's dmax^2 and displacement sums (in this rank's copy of pos4) and drift[0..1] back to 0;
 * drift[2] = the margin of the wake lists of this binning (list_adapt: from the largest dmax^2 found there before the reset). */
int gpd_swarm_bin(const GpdSwarm* swarm, void* stream);
/* Downwash forces of the rank's drones for the positions in pos4 -> dw_force, and drift[0..1] for the next gpd_swarm_step.
 * build_lists: non-zero on the call that follows a gpd_swarm_bin (ignored without wake lists). */
int gpd_swarm_forces(const GpdParams* params, const GpdSwarm* swarm, int32_t build_lists, void* stream);

/*
 * Neighbour queries: for every row of a query range, how many OTHER drones are closer than `radius`, and the nearest k of them.
 * Replaces BaseAviary._getAdjacencyMatrix (envs/BaseAviary.py:658-675: an O(N^2) Python loop over every pair of ONE aviary on
 * the host) for the batched aviaries, and gives the one-world swarm -- where a dense matrix is out of the question -- the
 * k-nearest lists a decentralised policy or a flocking rule observes, and a collision test (radius = two collision radii, k = 1).
 *
 *   pos4            [n_rows][4] floats x, y, z, (ignored), 16-byte aligned: GpdSwarm.pos4, or plane P of GpdState.kin.  A row
 *                   whose position is not finite takes no part, neither as query nor as neighbour (GpdSwarm's rows without a
 *                   drone and its meta rows are such rows)
 *   query_first, query_count   the rows that are answered (a rank of a shared world asks for its own slab); all rows can be neighbours
 *   radius          > 0, finite.  Neighbour: 3-D Euclidean distance STRICTLY below it (:673) -- squared distances
 *                   (dx*dx + dy*dy) + dz*dz in fp32 against radius^2 computed in float64 and rounded once
 *   k               1 .. 32 entries per query
 *   drones_per_env  0: ONE world.  The rows are sorted by the cell of a periodic x-y grid laid over the box x0 <= x <= x1,
 *                   y0 <= y <= y1 (the counting sort of gpd_downwash_global) and a query searches the 3 x 3 cells around its
 *                   own.  Cell size: max(cell, radius * 65/64) -- `cell` = 0 asks for the smallest -- doubled until nx * ny <= 65536;
 *                   nx, ny >= 3.  Drones outside the box wrap around (still exact: every pair is distance-tested, and the 1/64
 *                   covers the fp32 rounding of the cell coordinates up to 65 536 cells from the corner).  The cell size, the
 *                   box and visit_order change the speed, never the result.
 *                   D = 2 .. 256: n_rows / D independent aviaries of D consecutive rows, neighbours inside the aviary only; no
 *                   grid, no scratch (cell .. sorted_xyzc ignored); n_rows, query_first and query_count are multiples of D.
 *   visit_order, cell_count, cell_start, order, sorted_xyzc   (one world) the sort's scratch as for gpd_downwash_global, no
 *                   allocation inside the library: visit_order [n_rows] or NULL; cell_count [2 * 65537] int32, ZERO before the
 *                   first call and left zeroed by every call; cell_start [65537] int32; order [n_rows] int32 (out: the sorted
 *                   order, a permutation of the rows -- next call's visit_order, ping-pong); sorted_xyzc [n_rows][4] float
 *   nbr_count       [query_count] int32 out: neighbours of the row, however many (may exceed k) = the row sum of the
 *                   reference's matrix minus its diagonal 1
 *   nbr_idx         [query_count][k] int32 out or NULL: the min(k, count) nearest, ordered by (squared distance, row) ascending --
 *                   ties go to the lower row, whatever order the sort left the candidates in; the rest -1.  One world: row
 *                   numbers of pos4; drones_per_env = D: the drone's index inside its aviary
 *   nbr_rel         [query_count][k][4] float out or NULL (16-byte aligned): (xj - xi, yj - yi, zj - zi, distance) of those
 *                   entries; padding (0, 0, 0, +inf)
 *   adjacency       [query_count / D][D][D] uint8 out or NULL, drones_per_env = D only: the reference's matrix, diagonal 1
 * Everything is validated before the first device call: GPD_EINVAL (NULL pos4 / nbr_count / scratch, radius, alignment,
 * drones_per_env, adjacency with one world, box, cell), GPD_ERANGE (k, the query range).  Asynchronous on `stream`; three or
 * four launches for one world (count, [scan,] scatter, search), one for aviaries.
 */
int gpd_neighbors(const float* pos4, int32_t n_rows, int32_t query_first, int32_t query_count, float radius, int32_t k,
                  int32_t drones_per_env, float cell, float x0, float y0, float x1, float y1, const int32_t* visit_order,
                  int32_t* cell_count, int32_t* cell_start, int32_t* order, float* sorted_xyzc, int32_t* nbr_count,
                  int32_t* nbr_idx, float* nbr_rel, uint8_t* adjacency, void* stream);

/*
 * Obstacle fields: for every drone the signed distance to the nearest obstacle and its direction, whether it collides, and what
 * a fan of range sensors sees.  The reference puts bodies into the Bullet world (BaseAviary._addObstacles, envs/BaseAviary.py:
 * 958-981; BaseRLAviary._addObstacles, envs/BaseRLAviary.py:99-128) and leaves every question about them to Bullet; here the
 * world is a list of analytic shapes and the questions are answered on the device.  Nothing acts on the integrator: a consumer
 * combines `hit` into its own termination, or steers by the normals.
 *
 * An obstacle is a record of GPD_OBST_FLOATS = 8 floats  cx, cy, cz, kind, ax, ay, az, 0  (kind: a GPD_OBST_* value stored
 * exactly in a float):
 *   GPD_OBST_NONE      skipped (lists of different lengths per aviary are padded with it)
 *   GPD_OBST_SPHERE    centre c, radius ax
 *   GPD_OBST_BOX       axis-aligned, centre c, half extents ax, ay, az
 *   GPD_OBST_CYLINDER  vertical, centre c, radius ax, half height az
 *   GPD_OBST_FLOOR     the half-space z <= cz
 * The formulas are csrc/obstacle_math.inc: the exact signed distance (negative inside) with its unit gradient, and the first entry
 * t >= 0 of a ray p + t d, |d| = 1 (t = 0 for an origin inside or on the obstacle, +inf for a miss).
 *
 *   pos4            [n][4] floats x, y, z, (ignored), 16-byte aligned: plane P of GpdState.kin, or GpdSwarm.pos4 (as gpd_neighbors)
 *   quat4           [n][4] floats x, y, z, w, 16-byte aligned: plane Q of GpdState.kin; NULL when no ray needs it (ray_frame 0)
 *   drones_per_env  D >= 1: row i belongs to aviary i / D (n is a multiple of D).  0: one world
 *   obst, n_obst, obst_ld   float f of record m of aviary e is obst[(m * 8 + f) * obst_ld + e]:  obst_ld = 1 is ONE list of n_obst
 *                   records ([n_obst][8], e = 0) shared by every drone; obst_ld >= n / D is one list per aviary, stored as field
 *                   planes (needs D >= 1).  1 <= n_obst <= GPD_OBST_MAX
 *   collision_radius   the drone as a SPHERE of this radius (COLLISION_R of the airframe): the URDF's collision body is a cylinder of
 *                   that radius and of height COLLISION_H, which the sphere approximates -- it is exact sideways and generous by
 *                   COLLISION_R - COLLISION_H / 2 above and below
 *   clear4          [n][4] float out or NULL (16-byte aligned): (nx, ny, nz, d) -- d the minimum over the records of each one's own
 *                   signed distance, n that record's unit gradient (away from the obstacle)
 *   nearest         [n] int32 out or NULL: the minimising record; ties go to the lower m
 *   hit             [n] uint8 out or NULL: 1 where d < collision_radius (strictly)
 *                   Every record NONE, or a position that is not finite: (0, 0, 0, +inf), nearest -1, hit 0.
 *   ray_dirs, n_rays   [n_rays][3] unit vectors shared by all drones, 1 <= n_rays <= GPD_OBST_MAX_RAYS (read only with `ranges`)
 *   ray_frame       GPD_RAY_WORLD: the directions as they are.  GPD_RAY_LEVEL: rotated about z by the drone's yaw (the yaw of
 *                   pybullet's Euler angles of the NORMALISED quaternion).  GPD_RAY_BODY: rotated by the attitude; |q| does not
 *                   matter (DYN never renormalises q)
 *   max_range       > 0, finite
 *   ranges          [n][n_rays] float out or NULL (then every ray argument is ignored): the smallest entry distance over the records,
 *                   capped at max_range; no hit is max_range
 *   ray_hit         [n][n_rays] int32 out or NULL: the record that was hit (ties to the lower m), -1 for none within max_range
 *                   A pose that is not finite (position; the quaternion where the frame uses it): max_range and -1.
 * Everything is validated before the first device call.  GPD_EINVAL: NULL pos4 / obst, no output at all, alignment, n <= 0, n not a
 * multiple of D, obst_ld, and with `ranges`: NULL ray_dirs, max_range, ray_frame, NULL quat4 for the frames that need it.
 * GPD_ERANGE: n_obst, n_rays, n > 2^26.  Asynchronous on `stream`, no allocation, at most two launches (clearance; scan).
 */
enum { GPD_OBST_NONE = -1, GPD_OBST_SPHERE = 0, GPD_OBST_BOX = 1, GPD_OBST_CYLINDER = 2, GPD_OBST_FLOOR = 3 };
enum { GPD_RAY_WORLD = 0, GPD_RAY_LEVEL = 1, GPD_RAY_BODY = 2 };
#define GPD_OBST_FLOATS 8
#define GPD_OBST_MAX 1024
#define GPD_OBST_MAX_RAYS 64
int gpd_obstacles(const float* pos4, const float* quat4, int32_t n, int32_t drones_per_env, const float* obst, int32_t n_obst,
                  int64_t obst_ld, float collision_radius, float* clear4, int32_t* nearest, uint8_t* hit, const float* ray_dirs,
                  int32_t n_rays, int32_t ray_frame, float max_range, float* ranges, int32_t* ray_hit, void* stream);

/*
 * Obstacle courses as a task: gpd_rollout with the obstacle list inside the step.  num_steps = 1 is the env.step() of an
 * obstacle-avoidance environment, num_steps = K its rollout; one launch either way.  The reference gestures at such a task with
 * BaseRLAviary._addObstacles (envs/BaseRLAviary.py:99-128) and never scores it.  Per step and drone, in this order:
 *   1. the env step exactly as gpd_rollout takes it (action mapping, `substeps` sub-steps, the rpy refresh, the task's reward and flags);
 *   2. the clearance of the position the step reached, as gpd_obstacles computes it: d the minimum over the records of each one's
 *      signed distance (ties to the lower record), n that record's gradient; (0, 0, 0, +inf) without a live record or a finite
 *      position;  hit = d < collision_radius;
 *   3. (csrc/obst_task_math.inc)  reward = task_reward + hit_reward * hit - prox_weight * max(0, prox_margin - (d - collision_radius)),
 *      terminated |= hit_terminates & hit,  collided = hit;
 *   4. with cfg.auto_reset, the same-step reset on terminated | truncated, as gpd_step does it (the pose and its rpy restored, the
 *      rates, last_clipped_action and the step counter zeroed; the DSLPID members survive);
 *   5. the observation row of the state the step LEAVES BEHIND -- of the reset pose where the aviary was reset, clearance included:
 *      pos rpy vel ang_v | nx ny nz d | range_0 .. range_{n_rays - 1}  (16 + n_rays floats), each range the smallest entry of
 *      gpd_obstacles' ray over the records, capped at max_range, the directions turned by ray_frame as gpd_obstacles turns them.
 *
 *   params, state, cfg, actions, action_step_stride, target_pos, init_pose   as gpd_rollout (a stride of 0 holds one block)
 *   task            GpdObstTask: collision_radius > 0 (the drone as a sphere, as in gpd_obstacles), hit_terminates 0 / 1, hit_reward
 *                   (finite), prox_margin and prox_weight (>= 0), n_rays 0 .. GPD_OBST_MAX_RAYS, ray_frame GPD_RAY_*, max_range > 0
 *                   (the last two are read only when n_rays > 0); every float finite
 *   obst, n_obst, obst_ld   the records of gpd_obstacles: obst_ld = 1 one shared list [n_obst][8], obst_ld >= num_envs field planes
 *                   per aviary; 1 <= n_obst <= GPD_OBST_MAX
 *   ray_dirs        [n_rays][3] unit vectors (NULL allowed with n_rays = 0)
 *   rows            out, 16-byte aligned: row of drone n at step t at rows + t * row_step_stride + n * row_ld; row_ld a multiple of 4
 *                   and >= 16 + n_rays, row_step_stride a multiple of 4 (floats past 16 + n_rays of a row are not written)
 *   reward, terminated, truncated, collided   [num_envs] per step, env_step_stride elements apart
 * The state, the step counters, last_rpm and the DSLPID members are written back once per launch.
 * Supported: drones_per_env == 1; GPD_ACT_RPM, GPD_ACT_VEL, GPD_ACT_PID; GPD_TASK_NONE and GPD_TASK_HOVER; physics_flags 0 or any of
 * GPD_PHYS_GND | DRAG | GROUND | DAMP.  GPD_ENOTSUP, before any device call: drones_per_env > 1, another action type,
 * GPD_TASK_MULTIHOVER, GPD_PHYS_DW, state.bad or state.act_ring non-NULL.  GPD_EINVAL: a NULL pointer, the state's layout, sizes and
 * strides, unknown enums, the task's values, the rows' alignment and pitch, obst_ld, whatever the configuration needs and misses
 * (state.pid, state.last_rpm, target_pos, init_pose).  GPD_ERANGE: n_obst, n_rays, more than 2^26 drones.  Asynchronous on `stream`,
 * no allocation, one launch.  There is no collision RESPONSE: a drone that is not reset flies on through the obstacle.
 */
typedef struct GpdObstTask {
    float   collision_radius;          /* > 0, finite: the drone as a sphere, as in gpd_obstacles */
    int32_t hit_terminates;            /* 0 / 1: terminated |= hit */
    float   hit_reward;                /* added to the reward of the step that ends in contact (finite) */
    float   prox_margin, prox_weight;  /* >= 0, finite: reward -= prox_weight * max(0, prox_margin - (d - collision_radius)) */
    int32_t n_rays;                    /* 0 .. GPD_OBST_MAX_RAYS */
    int32_t ray_frame;                 /* GPD_RAY_* */
    float   max_range;                 /* > 0, finite (read only when n_rays > 0) */
} GpdObstTask;
int gpd_sizeof_obst_task(int32_t* size_out);
int gpd_rollout_obst(const GpdParams* params, const GpdState* state, const GpdStepCfg* cfg, const GpdObstTask* task, int32_t num_steps,
                     const float* actions, int64_t action_step_stride, const float* target_pos, const float* init_pose,
                     const float* obst, int32_t n_obst, int64_t obst_ld, const float* ray_dirs,
                     float* rows, int64_t row_ld, int64_t row_step_stride,
                     float* reward, uint8_t* terminated, uint8_t* truncated, uint8_t* collided, int64_t env_step_stride,
                     void* stream);

/*
 * Sampling-based model-predictive control (MPPI, Williams et al., "Information theoretic MPC for model-based reinforcement
 * learning", ICRA 2017): per drone, M perturbed action sequences around a nominal one are rolled H env steps through the physics,
 * scored, and the nominal is replaced by their cost-weighted average.  The reference has no planner; the nearest it comes is the
 * hand-written DSLPID set-points of its examples.  One launch; the state is READ ONLY -- the call leaves every byte of GpdState as
 * it found it -- and the M x H trajectories never reach memory.
 *
 * For drone n, sample m, step h:
 *   z     the four standard normals of (n, m, h, iteration): Philox4x32-10 with key `seed` on the counter (n, m, h, iteration), its
 *         four words as the float32 uniforms ((x >> 8) + 0.5) 2^-24 in (0, 1], two Box-Muller pairs (csrc/mppi_math.inc)
 *   a     clamp(u_in[h][n] + sigma o z, act_lo, act_hi), per component
 *   step  one env step exactly as gpd_rollout takes it for the action a (the action mapping with DSLPID and its members for
 *         GPD_ACT_VEL, `substeps` sub-steps, the rpy refresh); controller members and kinematic state are per-sample copies
 *   c_h   of the state AFTER the step:  w_pos |p - goal_h|^2 (x w_term at h = H - 1) + w_vel |v|^2 + w_tilt (1 - R22)
 *         + w_rate |omega_body|^2 + w_obs max(0, obst_margin - (d - collision_radius))^2,  d the minimum of the records' signed
 *         distances (csrc/obstacle_math.inc; the term is absent without a list), R22 of the quaternion as it is.  Every term is
 *         continuous in the state.
 * S_m = sum_h c_h;  w_m = exp(-(S_m - min S) / lambda), minimum and sums over the FINITE S_m only, a sample whose cost is not finite
 * has weight 0;  u_out[h] = u_in[h] + sum_m w_m (a_mh - u_in[h]) / sum_m w_m, clamped once more against rounding.  No finite sample
 * at all: u_out = clamp(u_in), stats4 = (+inf, +inf, 0, 0) -- what a drone whose start state is not finite gets, every one of its costs
 * being NaN or +-inf.  Finite costs up to FLT_MAX (w_obs as a hard wall: the hinge of a sample that comes too close overflows to +inf,
 * the others stay large and finite) are averaged without overflow: the sums are taken over w and w (S 2^-11).
 *
 *   cfg             drones_per_env = 1, physics_flags 0 (the planning model is the flag-less explicit integrator), task GPD_TASK_NONE,
 *                   no auto-reset, act_type GPD_ACT_RPM or GPD_ACT_VEL; any sub-step count
 *   u_in, u_step_stride     [H][N][4] nominal actions, 16-byte aligned, the stride in floats (a multiple of 4, >= 4 N)
 *   goal, goal_step_stride  [N][4] x, y, z, (ignored), 16-byte aligned; stride 0: one goal per drone for every step, else [H][N][4]
 *   obst, n_obst, obst_ld   the records of gpd_obstacles; NULL or n_obst 0: no list.  obst_ld 0: ONE list [n_obst][8] shared by every
 *                   drone; obst_ld >= N: one list per aviary as field planes, float f of record r of aviary e at
 *                   obst[(r * 8 + f) * obst_ld + e]
 *   u_out           [H][N][4] out, the stride of u_in; must not be u_in
 *   costs           [N][M] out, REQUIRED: S_m per sample -- also the kernel's workspace between its two passes
 *   stats4          [N][4] out, 16-byte aligned: min S, the weighted mean sum w S / sum w, the effective sample size
 *                   (sum w)^2 / sum w^2, the number of samples with a finite cost
 * Refused before any device work.  GPD_EINVAL: a NULL pointer (obst excepted), the state's layout, samples not a multiple of 64 in
 * 64 .. 1024, horizon < 1, lambda not positive and finite, a sigma that is negative or not finite, act_lo > act_hi, u_out == u_in,
 * alignment, the strides, n_obst outside 0 .. GPD_OBST_MAX, obst_ld neither 0 nor >= N, GPD_ACT_VEL without state.pid.
 * GPD_ENOTSUP: drones_per_env != 1, any physics flag, a task or auto_reset, any other action type, GPD_ACT_VEL on an airframe
 * without DSLPID.  GPD_ERANGE: N > 2^26.  Asynchronous on `stream`, no allocation, one launch; two calls with the same arguments
 * give the same bits.
 */
typedef struct GpdMppi {
    int32_t horizon;        /* H >= 1 env steps */
    int32_t samples;        /* M: a multiple of 64, 64 .. 1024 */
    float sigma[4];         /* std of the noise per action component (>= 0) */
    float act_lo[4], act_hi[4];   /* a = clamp(u + sigma*z, lo, hi) per component */
    float lambda;           /* temperature > 0 */
    float w_pos, w_vel, w_tilt, w_rate;   /* running cost */
    float w_term;           /* the position term of the LAST step is multiplied by this */
    float w_obs, obst_margin;             /* hinge on the clearance */
    float collision_radius;
    uint32_t seed[2];       /* Philox key */
    uint32_t iteration;     /* fourth counter word: the caller bumps it per plan */
} GpdMppi;
int gpd_mppi(const GpdParams* params, const GpdState* state, const GpdStepCfg* cfg, const GpdMppi* mppi, const float* u_in,
             int64_t u_step_stride, const float* goal, int64_t goal_step_stride, const float* obst, int32_t n_obst, int64_t obst_ld,
             float* u_out, float* costs, float* stats4, void* stream);

/*
 * gpd_mppi over thrust and body-rate commands (struct GpdCtbr and gpd_rollout_ctbr, below): the semantics of gpd_mppi word for word --
 * noise, clamp, cost terms, softmax over the finite costs, u_out, costs, stats4, strides, obstacle lists, struct GpdMppi -- except
 *   a     a CTBR command: thrust [m/s^2], then body rates x, y, z [rad/s]; clamp(u_in[h][n] + sigma o z, act_lo, act_hi) as above
 *   step  one control step exactly as gpd_rollout_ctbr takes it in GPD_CTBR_CMD with physics_flags 0 and no plant table: the command
 *         is held, and in every one of `substeps` sub-steps the rate loop (csrc/ctbr_math.inc, the controller's M and J those of
 *         `params`) gives the RPMs from the integrator's own body rates.  The rate loop clips the command to [0, thrust_max] and
 *         +-rate_max and the rotor thrusts to [0, f_max]: bounds wider than the clips are legal and act as the clips.
 * state.last_rpm is not read (no drag), nothing of GpdState is written.
 *   ctbr            HOST pointer, like GpdParams
 *   cfg             as for gpd_mppi, but act_type GPD_ACT_RAW_RPM or GPD_ACT_DIRECT_RPM, as gpd_rollout_ctbr has it
 * Refused before any device work, every message starting "gpd_mppi_ctbr: ".  GPD_EINVAL: everything gpd_mppi answers with it
 * (state.pid is never needed), and NULL ctbr.  GPD_ENOTSUP: drones_per_env != 1, any physics flag, a task or auto_reset, any other
 * action type.  GPD_ERANGE: N > 2^26.  Asynchronous on `stream`, no allocation, one launch; two calls with the same arguments give
 * the same bits.  DESIGN.md section 3.19.
 */
struct GpdCtbr;
int gpd_mppi_ctbr(const GpdParams* params, const struct GpdCtbr* ctbr, const GpdState* state, const GpdStepCfg* cfg, const GpdMppi* mppi,
                  const float* u_in, int64_t u_step_stride, const float* goal, int64_t goal_step_stride, const float* obst, int32_t n_obst,
                  int64_t obst_ld, float* u_out, float* costs, float* stats4, void* stream);

/*
 * MPPI that keeps away from moving PEERS -- the other drones of one airspace, and other moving bodies: gpd_mppi (ctbr NULL: its model
 * and action types) or gpd_mppi_ctbr (ctbr given: its model and action types) word for word -- noise, clamp, model step, the other
 * cost terms, softmax over the finite costs, u_out, costs, stats4, strides, obstacle lists, a state that is only read -- with one more
 * term in the running cost and one more output.  The N single-drone aviaries are taken to share one airspace.
 *   c_h  += w_peer * sum over the counted entries j = 0 .. k-1 of drone n's row of `idx`, in that order, of
 *           max(0, peer_dist - |p - pos[h][idx[n][j]]|)^2        (csrc/mppi_peers_math.inc), p the sample's position AFTER step h,
 *         added after the other terms' sum.  An entry < 0, >= n_rows or equal to n is not counted (and ends nothing: later entries
 *         count); a row of pos that is not finite adds 0; a peer at p itself adds peer_dist^2.  The term is continuous and C1 in p.
 *         With no counted entry, or w_peer = 0, u_out, costs and stats4 are those of gpd_mppi / gpd_mppi_ctbr bit for bit.
 *   pos, pos_step_stride   [H][n_rows][4] x, y, z, (ignored), 16-byte aligned: where row r is AFTER step h (a peer's path_out of an
 *         earlier call, or any prediction); rows 0 .. N-1 are the planned drones, rows beyond them other bodies.  Stride 0: ONE row
 *         set [n_rows][4] for every step (peers held where they are); else a multiple of 4 floats, >= 4 n_rows
 *   idx, k, idx_ld         [N][idx_ld] int32, 1 <= k <= 32 entries read per drone (the k-nearest lists of gpd_neighbors, -1 padded,
 *         are such rows)
 *   path_out   [H][N][4] out or NULL, the layout and stride of u_out, 16-byte aligned; must not be u_in or u_out, and must not
 *         overlap pos.  After the update the NEW nominal -- u_out as stored, the clamped one -- is flown without noise from the
 *         start state through the same model: x, y, z the position after step h, w the distance to the nearest counted peer at
 *         that step (+inf: none).  One writer per row.  A drone whose start state is not finite: x, y, z are those of the flight
 *         from that state, some component not finite at every step, and w is +inf (a distance that is not finite is no peer's).
 * Refused before any device work, every message starting "gpd_mppi_peers: ".  GPD_EINVAL: everything the model's own entry answers
 * with it, and NULL peers / idx / pos, k outside 1 .. 32, idx_ld < k, n_rows < N, a pos_step_stride that is neither 0 nor a multiple
 * of 4 >= 4 n_rows, a misaligned pos or path_out, path_out equal to u_in or u_out, w_peer or peer_dist negative or not finite.
 * GPD_ENOTSUP, GPD_ERANGE: as the model's own entry.  Asynchronous on `stream`, no allocation, one launch, no atomics; two calls
 * with the same arguments give the same bits.  DESIGN.md section 3.20.
 */
typedef struct GpdMppiPeers {
    const int32_t* idx;       /* device [N][idx_ld]: rows of `pos` to keep away from; an entry < 0, >= n_rows, or equal to the drone's own row n is skipped (not a terminator) */
    const float*   pos;       /* device [H][n_rows][4] x, y, z, (ignored), 16-byte aligned: where row r is AFTER step h; rows 0 .. N-1 are the planned drones, rows beyond them other moving bodies */
    float*         path_out;  /* device [H][N][4] or NULL, the layout and stride of u_out: see above */
    int64_t pos_step_stride;  /* floats; 0: one table row set for every step (peers held where they are), else a multiple of 4, >= 4 n_rows */
    int32_t k, idx_ld;        /* 1 <= k <= 32 (neighbors.MAX_K), idx_ld >= k */
    int32_t n_rows;           /* >= N */
    float w_peer, peer_dist;  /* c_h += w_peer * sum over the counted entries j = 0 .. k-1, in that order, of max(0, peer_dist - |p - pos[h][idx[n][j]]|)^2 */
} GpdMppiPeers;
int gpd_mppi_peers(const GpdParams* params, const struct GpdCtbr* ctbr /* NULL: gpd_mppi's model and action types; else gpd_mppi_ctbr's */,
                   const GpdState* state, const GpdStepCfg* cfg, const GpdMppi* mppi, const GpdMppiPeers* peers, const float* u_in,
                   int64_t u_step_stride, const float* goal, int64_t goal_step_stride, const float* obst, int32_t n_obst, int64_t obst_ld,
                   float* u_out, float* costs, float* stats4, void* stream);

/*
 * MPPI on the AVIARY'S OWN MODEL: gpd_mppi (ctbr NULL: its model and action types) or gpd_mppi_ctbr (ctbr given: its model and action
 * types) word for word -- noise, clamp, cost terms, softmax over the finite costs, u_out, costs, stats4, strides, obstacle lists, struct
 * GpdMppi, a state that is only read -- except the model step, which flies every drone's own airframe under the force terms of
 * cfg.physics_flags, as gpd_rollout_plant / gpd_rollout_ctbr fly it.
 *   plant_rows   NULL (the nominal airframe), or the per-drone plant table of gpd_plant_derive ([GPD_PLANT_ROWS][state.ld], 16-byte
 *         aligned): drone n's model is column n.  One wave plans one drone, so its row is read once, at wave-uniform addresses.  The
 *         controller (DSLPID's model and gains, the rate loop's M and J), the action mapping (HOVER_RPM, the MAX_RPM clip), the
 *         geometry, gnd_eff_h_clip and ground_z stay nominal, exactly as the plant path defines it (GPD_PLANT_*, above).
 *   cfg.physics_flags   any of GPD_PHYS_GND, GPD_PHYS_DRAG, GPD_PHYS_GROUND, GPD_PHYS_DAMP.  (Under GPD_PHYS_GROUND a start height of -inf is below
 *         the plane: the first sub-step of every sample puts the drone on it, and it plans like any other.)
 *   step  ctbr NULL: one env step as gpd_step takes it for one drone -- the action mapped on the plant, then `substeps` sub-steps; the drag
 *         term sees the previous step's RPMs on the first sub-step and this step's after it, and the last RPMs are carried from step to
 *         step of a sample.  ctbr given: one control step as gpd_rollout_ctbr takes it in GPD_CTBR_CMD -- the rate loop on the nominal M
 *         and J, the rotor thrusts and the sub-step on the plant, the drag term on the RPMs applied one sub-step earlier.
 *         A sample's first "previous RPMs" are state.last_rpm, required with GPD_PHYS_DRAG as everywhere else.
 * With plant_rows NULL and no flag the call equals the model's own entry bit for bit; so does a table of all-ones scales.
 * Refused before any device work, every message starting "gpd_mppi_plant: ".  Everything the model's own entry refuses, with the same
 * code (a physics flag other than GPD_PHYS_DW is legal here); GPD_ENOTSUP: GPD_PHYS_DW or state.dw_force (downwash needs mates);
 * GPD_EINVAL: GPD_PHYS_DRAG without state.last_rpm, plant_rows not 16-byte aligned.  Asynchronous on `stream`, no allocation, one launch,
 * no atomics; two calls with the same arguments give the same bits.  DESIGN.md section 3.21.
 */
int gpd_mppi_plant(const GpdParams* params, const struct GpdCtbr* ctbr /* NULL: gpd_mppi's model and action types; else gpd_mppi_ctbr's */,
                   const GpdState* state, const GpdStepCfg* cfg, const GpdMppi* mppi,
                   const float* plant_rows /* [GPD_PLANT_ROWS][state->ld] as gpd_rollout_plant reads them; NULL: the nominal airframe */,
                   const float* u_in, int64_t u_step_stride, const float* goal, int64_t goal_step_stride, const float* obst, int32_t n_obst,
                   int64_t obst_ld, float* u_out, float* costs, float* stats4, void* stream);

/*
 * Masked reset. Replaces BaseAviary.reset/_housekeeping (envs/BaseAviary.py:220-255, 451-477)
 * for the envs whose mask byte is non-zero (mask == NULL: all).  Sets pos/quat to init_pose,
 * vel, rpy_rates, last_rpm and step_counter to zero and writes the initial obs12 rows.  As in
 * the reference, the DSLPID state is NOT reset unless reset_pid != 0.
 */
int gpd_reset(const GpdState* state, const float* init_pose, int32_t init_per_env,
              const uint8_t* mask, int32_t num_envs, int32_t drones_per_env, int32_t reset_pid,
              float* obs12, void* stream);

/*
 * Batched DSLPIDControl.computeControl (control/DSLPIDControl.py:82-145) for n independent
 * controllers.  Inputs are row-major [n][3] / [n][4] arrays; `pid` is the [9][ld] controller
 * state (updated in place).  target_rpy / target_vel / target_rpy_rates may be NULL (= zeros,
 * the reference's defaults).  Outputs: rpm [n][4], pos_e [n][3] (may be NULL), yaw_e [n]
 * (may be NULL; computed_target_rpy[2] - cur_rpy[2]).
 * Singular inputs -- a desired force of exactly zero, or one parallel to the target heading -- make the reference divide by zero and
 * return NaN RPMs and NaN attitude integrals.  Here every RPM and every member passes a clip, and a clip of a NaN returns one of its
 * bounds: the RPMs are finite and inside [rpm(MIN_PWM), rpm(MAX_PWM)], the nine members finite and inside their clips (which bound is
 * not specified), pos_e is target_pos - cur_pos as ever, yaw_e is not defined (it may be NaN).  The same holds for the DSLPID action
 * types inside gpd_step / gpd_rollout.
 */
int gpd_pid(const GpdParams* params, float* pid, int64_t ld, float ctrl_dt,
            const float* cur_pos, const float* cur_quat, const float* cur_vel,
            const float* target_pos, const float* target_rpy, const float* target_vel,
            const float* target_rpy_rates, float* rpm, float* pos_e, float* yaw_e,
            int32_t n, void* stream);

/*
 * gpd_pid, then a wait for it on `stream` (as gpd_step_sync waits: up to 64 controllers report through a page-locked word the
 * calling thread spins on, more take hipStreamSynchronize): the call behind the reference-shaped single-drone
 * `DSLPIDControl.computeControl` (control/DSLPIDControl.py:82-145 returns numpy values: every call ends in a host read), whose
 * operands and controller state live in page-locked host memory.  Same arguments and error codes as gpd_pid.
 */
int gpd_pid_sync(const GpdParams* params, float* pid, int64_t ld, float ctrl_dt,
                 const float* cur_pos, const float* cur_quat, const float* cur_vel,
                 const float* target_pos, const float* target_rpy, const float* target_vel,
                 const float* target_rpy_rates, float* rpm, float* pos_e, float* yaw_e,
                 int32_t n, void* stream);

/*
 * MRAC: the reference's model-reference adaptive controller (control/MRAC.py:12-155, flown by examples/mrac.py), batched, and fused
 * into the rollout.  State x = (pos, rpy, vel, body rates) of 12 floats, input u = (thrust, three torques).  The DESIGN
 * (control/MRAC.py:56-104 -- pole placement, the Lyapunov equation) is the host's business, in float64; the device receives its
 * products as fp32 constants, rounded once.  A HOST struct like GpdParams, passed by value in the kernel argument segment; the
 * kernels keep it in LDS.  All matrices row-major.
 */
typedef struct GpdMrac {
    float PB[48];           /* [12][4]  P Bm: the reference's  e^T P Bm  (:133-134) is  e^T PB */
    float Kr_ref_gain[48];  /* [4][12]  pinv(B) (A - B K):  rt = -Kr_ref_gain r         (:93, :128) */
    /* The reference model Am = A - B K, Bm = B (:95-96) in the form their structure allows (:69-85): B is zero above its last four
     * rows, so rows 0..7 of Am are those of A -- rows 0..5 are [0 I] (d/dt of pos, rpy = vel, body rates: nothing to store), rows 6, 7
     * hold gravity's four entries -- and only rows 8..11 are dense.  Evaluating the full 12 x 12 product adds exact zeros. */
    float Am_lo[48];        /* [4][12]  rows 8..11 of Am */
    float A_grav[4];        /* Am[6][3], Am[6][4], Am[7][3], Am[7][4] = g sin(psi), g cos(psi), -g cos(psi), g sin(psi) */
    float B_diag[4];        /* Bm[8+k][k] = 1/m, 1/Ixx, 1/Iyy, 1/Izz */
    float mixer[12];        /* [4][3]                                                   (:37-50) */
    float gamma_x, gamma_r; /* Gamma_x = gamma_x I, Gamma_r = gamma_r I                 (:99-100) */
    float inv_4kf;          /* 1/(4 KF), host-computed in float64                       (:144) */
    float max_torque;       /* 3200                                                     (:142) */
    float pwm2rpm_scale, inv_pwm2rpm_scale, pwm2rpm_const, min_pwm;                     /* (:30-33) */
    float max_pwm, pad_[3];
    /* read by gpd_mrac_reset only */
    float Kx0[48];          /* [12][4]  initial gains Kx = -K^T                         (:102) */
    float Kr0[16];          /* [4][4]   Kr = I                                          (:103) */
} GpdMrac;

/* Floats of controller state per controller: [GPD_MRAC_STATE][ld], controller n at mrac_state + r*ld + n (the state's SoA convention):
 * rows 0..47 Kx [12][4] row-major | rows 48..63 Kr [4][4] | rows 64..75 Xm. */
#define GPD_MRAC_STATE 76

/* sizeof(GpdMrac) -> *size_out, for a binding to verify its mirror.  (gpd_sizeof_swarm RETURNS its size; this one writes it and
 * returns 0, or GPD_EINVAL for NULL: like every entry with a pointer argument it answers NULL with a code.) */
int gpd_sizeof_mrac(int32_t* size_out);

/*
 * Batched MRAC.computeControl (control/MRAC.py:109-155) for n independent controllers, shaped like gpd_pid: one lane per
 * controller, asynchronous on `stream`, capturable.  In the reference's order: rpy of cur_quat; body rates = the intrinsic-XYZ
 * rotation of rpy, inverted, applied to cur_ang_vel (:121, restated as the reference computes it); Xm <- X where counter == 0,
 * counter += 1; rt = -Kr_ref_gain r; u = Kx^T X + Kr^T rt with the gains BEFORE this call's update; the adaptation
 * Kx += -gamma_x X (e^T PB) dt, Kr += -gamma_r rt (e^T PB) dt with e = X - Xm; thrust / torque clips, mixer and PWM clip;
 * Xm += (Am Xm + Bm rt) dt.
 *   mrac         HOST pointer, like GpdParams
 *   mrac_state   [GPD_MRAC_STATE][ld], updated in place;  counter [n] int32, updated in place
 *   cur_pos, cur_vel, cur_ang_vel [n][3], cur_quat [n][4] (16-byte aligned), target_pos [n][3]
 *   target_rpy, target_vel, target_rpy_rates   [n][3] or NULL (= zeros, the reference's defaults)
 *   rpm [n][4] out (16-byte aligned); pos_e [n][3], rpy_e [n][3] out or NULL (rpy_e: three angles, :150)
 * Validated before any device work.  GPD_EINVAL: a NULL pointer other than the optional ones, n <= 0 or ld < n, ctrl_dt <= 0,
 * cur_quat or rpm not 16-byte aligned.  GPD_ERANGE: n > 2^26 (32-bit byte offsets).
 */
int gpd_mrac(const GpdMrac* mrac, float* mrac_state, int32_t* counter, int64_t ld, float ctrl_dt,
             const float* cur_pos, const float* cur_quat, const float* cur_vel, const float* cur_ang_vel,
             const float* target_pos, const float* target_rpy, const float* target_vel, const float* target_rpy_rates,
             float* rpm, float* pos_e, float* rpy_e, int32_t n, void* stream);

/*
 * MRAC.reset (control/MRAC.py:106-107 -> BaseControl.reset) for the controllers whose mask byte is non-zero (mask == NULL: all):
 * the counter goes to zero and NOTHING else -- the next call re-seeds Xm from the state it sees, the adapted gains survive.
 * restore_gains != 0 (an extra the reference does not have) also puts Kx0 / Kr0 of `mrac` back (a second launch).
 * GPD_EINVAL: NULL mrac_state / counter, NULL mrac with restore_gains, n <= 0 or ld < n.  GPD_ERANGE: n > 2^26.
 */
int gpd_mrac_reset(float* mrac_state, int32_t* counter, int64_t ld, const GpdMrac* mrac, const uint8_t* mask, int32_t n,
                   int32_t restore_gains, void* stream);

/*
 * K control steps in ONE launch with the MRAC controller IN the loop: the loop of examples/mrac.py:82-90
 * (`obs, ... = env.step(action); action = ctrl.computeControlFromState(state=obs[0], ...)`).  A drone's state and its 76
 * controller floats are loaded once, stay in registers for all K steps and their sub-steps, and are stored once.  Step k: one env
 * step with the carried RPMs as the action (the first call of a fresh aviary: zeros, as the example starts), then one controller
 * call on the new state gives the next RPMs.  Bit for bit K x (gpd_step + gpd_mrac); K1 then K2 steps = K1 + K2 in one launch.
 *   cfg            drones_per_env = 1, task GPD_TASK_NONE, no auto-reset, act_type GPD_ACT_RAW_RPM or GPD_ACT_DIRECT_RPM, any
 *                  sub-step count; GPD_PHYS_GND / DRAG / GROUND / DAMP allowed, GPD_PHYS_DW (or state.dw_force): GPD_ENOTSUP (it
 *                  needs mates; gpd_step + gpd_mrac serve every shape)
 *   mrac_state, counter, mrac_ld   as in gpd_mrac, one controller per drone
 *   targets        step t reads [N][12] rows (target pos | rpy | vel | rpy rates) at targets + t*target_step_stride (floats);
 *                  stride 0 holds one block for all K steps.  16-byte aligned
 *   rpm_carry      [N][4] in/out, 16-byte aligned: the action of the first step in, the controller's latest output out
 *   plant_rows     NULL, or the per-drone plant table of gpd_plant_derive (pitch state.ld): the airframe is the drone's own while
 *                  `mrac` stays the nominal design
 *   obs12          step t writes [N][12] at obs12 + t*obs_step_stride; stride 0 keeps only the last step's rows.  16-byte aligned
 * Validated before any device work.
 *   GPD_EINVAL   a NULL pointer (plant_rows excepted), state.kin not 16-byte aligned or state.ld outside 1 .. 2^32 - 1, num_envs /
 *                substeps / num_steps <= 0, an unknown physics flag, state.ld or mrac_ld < num_envs, GPD_PHYS_DRAG without
 *                state.last_rpm, a negative step stride, a non-zero one below 12*num_envs or not a multiple of 4 floats, targets /
 *                rpm_carry / obs12 / plant_rows not 16-byte aligned, pyb_dt or ctrl_dt <= 0
 *   GPD_ENOTSUP  drones_per_env != 1, a task or auto_reset, an act_type other than the two RPM ones, GPD_PHYS_DW or state.dw_force
 *   GPD_ERANGE   num_envs > 2^26 (32-bit byte offsets)
 */
int gpd_rollout_mrac(const GpdParams* params, const GpdMrac* mrac, const GpdState* state, const GpdStepCfg* cfg,
                     float* mrac_state, int32_t* counter, int64_t mrac_ld, const float* targets, int64_t target_step_stride,
                     float* rpm_carry, const float* plant_rows, float* obs12, int64_t obs_step_stride, int32_t num_steps,
                     void* stream);

/*
 * CTBR: collective thrust and body rates, the reference's control/CTBRControl.py -- which it flies through BetaAviary with Betaflight as
 * the inner loop -- batched, and fused into the rollout with a rate loop of its own in place of the firmware.
 * A command is 4 floats: thrust as a mass-normalised acceleration [m/s^2], then the body rates x, y, z [rad/s].  The arithmetic of both
 * loops is csrc/ctbr_math.inc.  A HOST struct like GpdParams, passed by value in the kernel argument segment (wave-uniform).
 */
typedef struct GpdCtbr {
    /* the outer loop, CTBRControl.computeControl (:149-168): the reference's constants by default */
    float k_p[3];           /* K_P = (3, 3, 8) */
    float k_d[3];           /* K_D = (2.5, 2.5, 5) */
    float k_rates[3];       /* K_RATES = (5, 5, 1) */
    float g;                /* -G[2] = 9.8 (a constant of the reference's method, not the class's `g`) */
    /* the rate loop (new: the reference leaves it to the firmware), evaluated every physics sub-step */
    float k_rate[3];        /* [1/s], (40, 40, 20) by default */
    float thrust_max;       /* the command's clips: thrust to [0, thrust_max] (40.9 m/s^2) ... */
    float rate_max;         /* ... each rate to +-rate_max (360 deg/s), BetaAviary.ctbr2beta's limits (envs/BetaAviary.py:176-188) */
    float alloc[12];        /* [4][3]: f_i = M thrust / 4 + alloc[i] . tau, the exact inverse of the integrator's torque rows for the
                             * airframe (CF2X / RACE: +-1/(4 L/sqrt 2) | +-1/(4 kz); CF2P: +-1/(2 L), 0 | +-1/(4 kz); kz = +-KM/KF),
                             * host-computed in float64 */
    float f_max;            /* KF MAX_RPM^2: a rotor's thrust is clipped to [0, f_max] */
    float inv_kf;           /* 1/KF: rpm_i = sqrt(f_i / KF) */
    float pad_[3];          /* (to a multiple of 16 bytes) */
} GpdCtbr;

/* the two ways gpd_rollout_ctbr is commanded */
#define GPD_CTBR_CMD 0      /* rows are [N][4] commands */
#define GPD_CTBR_POS 1      /* rows are [N][12] targets (pos | rpy | vel | rpy rates): the outer loop runs in the kernel */

/* sizeof(GpdCtbr) -> *size_out, for a binding to verify its mirror (as gpd_sizeof_mrac).  GPD_EINVAL: NULL. */
int gpd_sizeof_ctbr(int32_t* size_out);

/*
 * Batched CTBRControl.computeControl (the outer loop alone) for n independent drones: one lane each, asynchronous on `stream`, capturable.
 *   ctbr         HOST pointer, like GpdParams
 *   cur_pos, cur_vel [n][3]; cur_quat [n][4], x y z w -- the state's order -- 16-byte aligned; target_pos [n][3]
 *   target_vel   [n][3] or NULL (= zeros, the reference's default).  The reference also accepts target_rpy and target_rpy_rates and
 *                ignores them; this entry does not take them
 *   cmd          [n][4] out, 16-byte aligned: thrust [m/s^2] | body rates [rad/s]
 * Validated before any device work.  GPD_EINVAL: a NULL pointer other than target_vel, n <= 0, cur_quat or cmd not 16-byte aligned.
 * GPD_ERANGE: n > 2^26 (32-bit byte offsets).
 */
int gpd_ctbr(const GpdCtbr* ctbr, const float* cur_pos, const float* cur_quat, const float* cur_vel, const float* target_pos,
             const float* target_vel, float* cmd, int32_t n, void* stream);

/*
 * K control steps in ONE launch with a body-rate loop closed INSIDE the physics sub-steps.  A drone's state is loaded once, stays in
 * registers for all K steps and their sub-steps, and is stored once.  A control step holds one command; every sub-step evaluates the rate
 * loop of ctbr_math.inc on the body rates the integrator carries and hands its four RPMs to the physics exactly as a
 * GPD_ACT_DIRECT_RPM action would.  The controller's M and J are those of `params` -- the nominal airframe -- with a plant table too.
 *   mode           GPD_CTBR_CMD: step t reads [N][4] commands at rows + t*row_step_stride (floats).  GPD_CTBR_POS: step t reads [N][12]
 *                  targets (pos | rpy | vel | rpy rates, gpd_rollout_mrac's layout; rpy and its rates are ignored, as the reference
 *                  does) and evaluates the outer loop on the state at the START of the control step.  Stride 0 holds one block for all
 *                  K steps.  16-byte aligned.  GPD_CTBR_POS is bit for bit K x (gpd_ctbr on the current state, GPD_CTBR_CMD with K = 1)
 *   cfg            as gpd_rollout_mrac: drones_per_env = 1, task GPD_TASK_NONE, no auto-reset, act_type GPD_ACT_RAW_RPM or
 *                  GPD_ACT_DIRECT_RPM (the two are the same here: the rate loop's RPMs are inside [0, MAX_RPM]), any sub-step count;
 *                  GPD_PHYS_GND / DRAG / GROUND / DAMP allowed
 *   state.last_rpm read for the drag term of the very first sub-step, written with the last sub-step's RPMs; the drag term of every
 *                  other sub-step sees the previous sub-step's RPMs (the reference's last_clipped_action rule, envs/BaseAviary.py:
 *                  359-372, carried to a controller that runs every sub-step).  The only state the controller carries
 *   plant_rows     NULL, or the per-drone plant table of gpd_plant_derive (pitch state.ld)
 *   obs12          step t writes [N][12] at obs12 + t*obs_step_stride; stride 0 keeps only the last step's rows.  16-byte aligned
 *   cmd_out        NULL, or [N][4] per step, 16-byte aligned: the commands each step flew, BEFORE the rate loop's clips, at
 *                  cmd_out + t*cmd_step_stride where cmd_step_stride is row_step_stride in GPD_CTBR_CMD (0: the held block, written K
 *                  times with what was read) and 4*num_envs in GPD_CTBR_POS.  Must not alias rows
 * K1 then K2 steps = K1 + K2 in one launch, bit for bit.  Validated before any device work.
 *   GPD_EINVAL   a NULL pointer (plant_rows, cmd_out excepted), state.kin not 16-byte aligned or state.ld outside 1 .. 2^32 - 1, num_envs /
 *                substeps / num_steps <= 0, an unknown physics flag or mode, state.ld < num_envs, GPD_PHYS_DRAG without state.last_rpm, a
 *                negative step stride, a non-zero one below a step's rows (4*num_envs or 12*num_envs for rows, 12*num_envs for obs12) or
 *                not a multiple of 4 floats, rows / obs12 / plant_rows / cmd_out not 16-byte aligned, cmd_out == rows, pyb_dt or
 *                ctrl_dt <= 0
 *   GPD_ENOTSUP  drones_per_env != 1, a task or auto_reset, an act_type other than the two RPM ones, GPD_PHYS_DW or state.dw_force
 *   GPD_ERANGE   num_envs > 2^26 (32-bit byte offsets)
 */
int gpd_rollout_ctbr(const GpdParams* params, const GpdCtbr* ctbr, const GpdState* state, const GpdStepCfg* cfg, int32_t mode,
                     const float* rows, int64_t row_step_stride, const float* plant_rows, float* obs12, int64_t obs_step_stride,
                     float* cmd_out, int32_t num_steps, void* stream);

/*
 * The single-drone task on rows: reward, terminated and truncated of num_envs single-drone aviaries from their obs12 rows, exactly as
 * gpd_step computes them inside the step (the same device function; envs/HoverAviary.py:68-132).  One lane per drone, asynchronous on
 * `stream`, capturable.  The building block that gives a composed flight -- gpd_rollout_ctbr, gpd_rollout_mrac -- a task.
 *   cfg          read: task, xy_bound, z_bound, tilt_bound, term_dist, trunc_counter, target_per_env, num_envs (drones_per_env must be 1)
 *   obs12        [num_envs][12], 16-byte aligned: position and roll / pitch are read from the row
 *   counter      [num_envs] int32: the aviary's step counter BEFORE the step's increment (what state.step_counter held before the step)
 *   target_pos   [3], or [num_envs][3] with target_per_env; NULL allowed with GPD_TASK_NONE
 *   reward [num_envs], terminated / truncated [num_envs] uint8 out.  GPD_TASK_NONE: -1, 0, 0, as gpd_step answers
 * With auto_reset = 0, gpd_step's obs12 rows and the counters from before the step give gpd_step's reward and flags bit for bit.
 * Validated before any device work.  GPD_EINVAL: a NULL pointer, num_envs <= 0, an unknown task, a task without target_pos, obs12 not
 * 16-byte aligned.  GPD_ENOTSUP: drones_per_env != 1, GPD_TASK_MULTIHOVER.  GPD_ERANGE: num_envs > 2^26.
 */
int gpd_task_eval(const GpdStepCfg* cfg, const float* obs12, const int32_t* counter, const float* target_pos, float* reward,
                  uint8_t* terminated, uint8_t* truncated, void* stream);

/*
 * CTBR as a task: the action of a single-drone aviary IS the thrust and body-rate command.  num_steps = 1 is the env.step() of such an
 * environment, num_steps = K its rollout; one launch either way.  Per step and drone, in env_step's order:
 *   1. the command: the [N][4] action row at actions + t*action_step_stride (stride 0 holds one block) as it is -- thrust [m/s^2], rates
 *      [rad/s] -- or, with task->normalized, cmd_i = fma(a_i, act_scale[i], act_bias[i]).  No clamp of its own: the rate loop's
 *      thrust_max / rate_max clips bound it;
 *   2. `substeps` sub-steps exactly as gpd_rollout_ctbr takes them (the same device function), then the rpy refresh;
 *   3. the task's reward and flags on the aviary's counter before the increment, as gpd_step computes them (GPD_TASK_NONE: -1, 0, 0);
 *   4. with cfg.auto_reset, the same-step reset on terminated | truncated, as gpd_step does it: the row of the finished episode goes to
 *      term_obs12, the pose and its rpy are restored (init_per_env 0 / 1), velocity, body rates, the observed angular velocity, the
 *      carried RPMs and the step counter become zero;
 *   5. the obs12 row of the state the step LEAVES BEHIND, reward / terminated / truncated.
 * Bit for bit what gpd_rollout_ctbr (GPD_CTBR_CMD, one step), gpd_task_eval on its rows with the counters from before the step, and
 * gpd_reset masked by terminated | truncated give; K1 then K2 steps = K1 + K2 in one launch.
 */
typedef struct GpdCtbrTask {
    float   act_scale[4];   /* normalized: cmd_i = fma(a_i, act_scale[i], act_bias[i]) -- hover-centred: (g, rate_max x 3) ... */
    float   act_bias[4];    /* ... and (g, 0, 0, 0): a = 0 is the hover command, a = -1 zero thrust */
    int32_t normalized;     /* 0: the action is the physical command, scale and bias are not read; 1: the affine map */
    int32_t pad_[3];        /* (to a multiple of 16 bytes) */
} GpdCtbrTask;

/* sizeof(GpdCtbrTask) -> *size_out, for a binding to verify its mirror (as gpd_sizeof_ctbr).  GPD_EINVAL: NULL. */
int gpd_sizeof_ctbr_task(int32_t* size_out);

/*
 *   params, ctbr, state, plant_rows   as gpd_rollout_ctbr.  state.bad, state.last_rpm and state.step_counter are written once per
 *                  launch, from the state the last step leaves (a drone reset in that step: its reset pose)
 *   cfg            drones_per_env = 1, GPD_TASK_NONE or GPD_TASK_HOVER, auto_reset 0 / 1, target_per_env and init_per_env 0 / 1,
 *                  act_type GPD_ACT_RAW_RPM or GPD_ACT_DIRECT_RPM, any sub-step count; GPD_PHYS_GND / DRAG / GROUND / DAMP allowed
 *   task           HOST pointer or NULL (= not normalized)
 *   target_pos     [3] or [N][3] (target_per_env); NULL allowed with GPD_TASK_NONE.  init_pose [7] or [N][7] (init_per_env): position,
 *                  quaternion x y z w; NULL allowed without auto_reset
 *   obs12          step t writes [N][12] at obs12 + t*obs_step_stride; stride 0 keeps only the last step's rows.  16-byte aligned
 *   term_obs12     NULL, or laid out as obs12: the rows of the drones whose episode ended at step t, before the reset; the other rows
 *                  are not written.  16-byte aligned, not obs12 itself.  With obs_step_stride = 0 it keeps, like obs12, the LAST
 *                  step only: an episode that ends at an earlier step of a K-step launch leaves no terminal row (give a stride to
 *                  keep every step's)
 *   reward [N] float, terminated / truncated [N] uint8 per step, env_step_stride elements apart; stride 0 keeps the last step only
 *   cmd_out        NULL, or [N][4] per step at cmd_out + t*action_step_stride, 16-byte aligned: the command flown, BEFORE the rate loop's
 *                  clips.  Must not alias actions
 * Validated before any device work.
 *   GPD_EINVAL   as gpd_rollout_ctbr, and: NULL actions / obs12 / reward / terminated / truncated, an unknown task, a task without
 *                target_pos, auto_reset without init_pose, a non-zero env_step_stride below num_envs, term_obs12 not 16-byte aligned or
 *                equal to obs12, cmd_out == actions, task->normalized neither 0 nor 1
 *   GPD_ENOTSUP  drones_per_env != 1, GPD_TASK_MULTIHOVER, an act_type other than the two RPM ones, GPD_PHYS_DW or state.dw_force,
 *                state.act_ring (the history would not be advanced)
 *   GPD_ERANGE   num_envs > 2^26 (32-bit byte offsets)
 * GPD_CTBR_POS targets are not offered as the action: a policy's action is the command.
 */
int gpd_rollout_ctbr_task(const GpdParams* params, const GpdCtbr* ctbr, const GpdState* state, const GpdStepCfg* cfg,
                          const GpdCtbrTask* task, int32_t num_steps, const float* actions, int64_t action_step_stride,
                          const float* target_pos, const float* init_pose, const float* plant_rows, float* obs12, float* term_obs12,
                          int64_t obs_step_stride, float* reward, uint8_t* terminated, uint8_t* truncated, int64_t env_step_stride,
                          float* cmd_out, void* stream);

/*
 * Gather the 20-float state vectors of BaseAviary._getDroneStateVector
 * (envs/BaseAviary.py:541-561): pos3 | quat4 | rpy3 | vel3 | ang_v3 | last_clipped_action4,
 * from the SoA state and the obs12 rows of the latest step.  state20 is [n][20].
 */
int gpd_state_vectors(const GpdState* state, const float* obs12, float* state20, int32_t n,
                      void* stream);

/*
 * The one optional exchange step of the multi-GPU layout: all-gather of the observation shards over RCCL (xGMI).
 * The aviaries shard across ranks with no data-path collective (one process per GPU, rank r owns a contiguous block of
 * envs); a centralised learner that wants the concatenated (E_total*D, 12) observation tensor -- what the reference's
 * single process holds in `obs` after `env.step()` (envs/BaseAviary.py:375, envs/BaseRLAviary.py:307-320; consumed by
 * examples/learn.py:157-192) -- gathers it with ONE collective per step (or per rollout: fewer, larger collectives).
 * RCCL is resolved at run time (dlopen of librccl.so.1; GPD_RCCL_LIB overrides): a single-GPU consumer needs no RCCL,
 * and GPD_ENOTSUP is returned when it cannot be found.
 *
 *   gpd_comm_unique_id   rank 0: ncclGetUniqueId; the caller distributes the GPD_COMM_ID_BYTES to the other ranks
 *                        (torch.distributed broadcast, MPI, a file ...)
 *   gpd_comm_init        every rank, after hipSetDevice: ncclCommInitRank (collective, blocks until all ranks joined)
 *   gpd_allgather_obs    ncclAllGather of `count` floats per rank: shard [count] -> full [world_size*count], rank r's
 *                        shard at full + r*count.  Asynchronous on `stream`, capturable in a hipGraph together with the
 *                        gpd_step / gpd_rollout launch that produced the shard.
 *   gpd_comm_count       ncclCommCount: the number of ranks RCCL itself says the communicator spans (a harness prints it
 *                        next to its throughput line: a run that silently fell apart into one-rank worlds shows here)
 *   gpd_comm_destroy     ncclCommDestroy (NULL is a no-op)
 * ONE communicator per process serves every count: create it once, pass any `count` to gpd_allgather_obs.
 * RCCL errors are returned as 1000 + ncclResult_t.
 */
#define GPD_COMM_ID_BYTES 128
int gpd_comm_unique_id(uint8_t id[GPD_COMM_ID_BYTES]);
int gpd_comm_init(void** comm, const uint8_t id[GPD_COMM_ID_BYTES], int32_t rank, int32_t world_size);
int gpd_comm_count(void* comm, int32_t* n_ranks);
int gpd_comm_destroy(void* comm);
int gpd_allgather_obs(void* comm, const float* shard, float* full, size_t count, void* stream);

/*
 * (ABI 8) Point-to-point exchange of float blocks between the ranks of a communicator, all operations of one call in ONE RCCL
 * group (ncclGroupStart, ncclSend / ncclRecv per block, ncclGroupEnd): the HALO exchange of a world shared by several ranks.
 * The reference's `_downwash` reads every other drone's position from the process's own arrays (envs/BaseAviary.py:798-811,
 * `self.pos[j]`); a rank of a sharded world needs the positions of the drones within the model's 10 m lateral cut-off (plus
 * a margin) of its own -- with the ranks holding stripes of the world, blocks from its two neighbours instead of the
 * all-gather of every position (gpd_allgather_obs in place; 16 B x every drone per sub-step).  xGMI is point to point: every
 * block travels over the one link between its two GPUs.
 *   sends / recvs   the operations: `count` floats at `ptr` to / from rank `peer`.  Several blocks between the same pair of
 *                   ranks are matched in the order they are listed (RCCL's rule); every send needs its receive on the peer,
 *                   in a call of its own made at the same point of the program.  Device pointers; asynchronous on `stream`,
 *                   capturable in a hipGraph.
 * GPD_ENOTSUP when RCCL (or its point-to-point entries) cannot be resolved.
 */
typedef struct GpdP2P {
    int32_t peer;          /* rank of the other side */
    int32_t pad_;
    void* ptr;             /* device pointer (send: read, receive: written) */
    int64_t count;         /* floats */
} GpdP2P;
int gpd_p2p_group(void* comm, const GpdP2P* sends, int32_t n_sends, const GpdP2P* recvs, int32_t n_recvs, void* stream);

/*
 * (ABI 8) Debug-bounds build.  A library compiled with -DGPD_DEBUG_BOUNDS (`python -c "from gym_pybullet_drones_amd import _native;
 * _native.build(debug=True)"` -> csrc/libgpd_debug.so; select it with GPD_LIB) checks every index its kernels READ FROM MEMORY before
 * they address with it, records the first violation and clamps the index, so that a corrupted ring position or wake list shows up
 * as a code instead of as an out-of-bounds access.  The reference has no counterpart (no sanitizer, no bounds
 * or race checks beyond numpy's own IndexError).  gpd_debug_status waits for `stream` and returns the record:
 *     out[0] code of the first violation (0: none), out[1] its workgroup, out[2] the offending value, out[3] violations so far;
 * reset != 0 clears the record.  A release build returns GPD_ENOTSUP (its kernels carry no checks).
 */
enum {
    GPD_DBG_RING_POS = 1,      /* GpdState.ring_pos outside [0, hist_len)          (gpd_step, gpd_rollout_history) */
    GPD_DBG_STEP_COUNTER = 2,  /* GpdState.step_counter negative */
    GPD_DBG_SLOT_ROW = 3,      /* GpdSwarm.order: sorted slot -> row outside [0, n_rows)   (gpd_swarm_forces) */
    GPD_DBG_SORT_KEY = 4,      /* GpdSwarm.slot_key outside the grid's keys */
    GPD_DBG_LIST_COUNT = 5,    /* GpdSwarm.pair_nb: more batches than list_cap */
    GPD_DBG_LIST_ENTRY = 6     /* GpdSwarm.pair_list: a candidate index outside [0, n_rows) */
};
int gpd_debug_status(uint32_t out[4], int32_t reset, void* stream);

/*
 * Diagnostics for the measurement harness (bench.py's issue roofline): runs a dependent v_fma_f32 chain at one wave per
 * SIMD and reports the shader clock it ran at [GHz] (shader-clock cycles / constant-rate wall-clock time) and, optionally,
 * the time per dependent FMA [ns].  Synchronous (it waits for `stream`).
 */
int gpd_clock_probe(double* shader_ghz, double* ns_per_fma, void* stream);

/*
 * The differentiable rollout (additions to ABI 9): analytic gradients through the K-step kernel, for policy gradients through the
 * physics and gradient-based trajectory optimisation.  The reference has no counterpart (its integrator is numpy,
 * envs/BaseAviary.py:815-892; nothing in it carries a derivative).
 *
 * gpd_rollout_tape is gpd_rollout (plant_rows == NULL: the nominal airframe) or gpd_rollout_plant (plant_rows given, pitch state.ld)
 * plus a record of what the reverse sweep needs.  Whatever it leaves behind -- state, last_rpm, step_counter, bad, obs12, reward and
 * flags -- is bit for bit what gpd_rollout / gpd_rollout_plant leaves on the same inputs (the same map_action / env_step / substep
 * code).  The tape is opaque, 16-byte aligned, gpd_rollout_tape_floats(cfg, num_steps, state.ld) floats: the 13 kinematic floats at
 * the start of every env step in the plane layout of GpdState.kin (52 B per drone-step) and one row for the rpm sum the drag term of
 * the call's first sub-step saw.
 *
 * gpd_rollout_vjp is the vector-Jacobian product of the map (kin_0, a_0 .. a_K-1) -> (kin_K, obs12_0 .., reward_0 ..) of that call:
 *   ld, num_steps, actions, action_step_stride, target_pos, plant_rows   what the taped call was given (ld = state.ld)
 *   g_obs12, g_reward   cotangents of the outputs, laid out like them (obs_step_stride / env_step_stride); NULL = zeros
 *   g_kin               [13*ld], the four-plane layout of GpdState.kin, IN PLACE: on entry the cotangent of the final state, on return
 *                       the cotangent of the initial state.  16-byte aligned
 *   g_actions           [K][N][A] out, ALWAYS one block per step -- also when action_step_stride == 0: the caller sums the blocks of
 *                       a shared action block.  16-byte aligned
 * One lane per drone, steps K-1 .. 0; with S sub-steps per step the forward sub-steps are re-run from the taped state for each
 * sub-step in reverse (S(S+1)/2 recomputations, no scratch memory).  No atomics: two calls give the same bits.  The adjoint is that
 * of the function as executed: a select differentiates the branch taken (the |w| ~ 0 test of the quaternion update, the gimbal
 * branches of the Euler extraction, the clip of GPD_ACT_RAW_RPM -- zero gradient outside its bounds --, max(0, .) of the reward).  The
 * observed world angular velocity uses the pre-update rotation and the post-update rates, and so does its adjoint.  The drag term of
 * a step's first sub-step sees the previous step's RPMs: inside one call that dependence is differentiated, the value carried in
 * from before the call is a constant.  Targets are constants of the sweep, and so are the plant rows in gpd_rollout_vjp.
 *
 * gpd_rollout_vjp_plant is gpd_rollout_vjp on a taped call that had a plant table (plant_rows != NULL, else GPD_EINVAL), and writes
 * g_kin and g_actions exactly as it does; the lane that walks the steps also sums, in registers, the cotangent of every plant row
 * the sweep reads and stores them once after the loop (no atomics):
 *   g_plant_rows        [GPD_PLANT_ROWS][ld] out, 16-byte aligned, drones 0 .. N-1 of every row overwritten: the cotangents of
 *                       INV_M, GRAVITY (it enters the total thrust and the weight), KF and HOVER_RESID (the raw RPM action types, at the
 *                       CLIPPED rpm), NORM_THRUST and NORM_GAP (the normalised action types), J[0..2] and J_INV[0..2] (independent rows,
 *                       as the forward reads them), KM_OVER_KF, DRAG[0..2].  Rows the supported configurations never read -- M, GND_EFF,
 *                       HOVER_THRUST, and the drag rows without GPD_PHYS_DRAG -- are exactly 0
 * gpd_plant_derive_vjp takes them to the nine scale factors: g_scales [GPD_NUM_SCALES][ld] (drones 0 .. n-1 overwritten) is the
 * transpose of gpd_plant_derive's Jacobian at `scales` applied to g_rows [GPD_PLANT_ROWS][ld], in double with one rounding per
 * output, e.g.  g_mass = M_n g_M - inv_M_n / s_mass^2 g_INV_M + GRAVITY_n g_GRAVITY + hover_thrust_n (g_HOVER_THRUST - g_HOVER_RESID
 * + g_NORM_GAP).  The action mapping's HOVER_RPM and the MAX_RPM clip are nominal and have no cotangent; targets and the RPMs carried
 * in from before the call stay constants.
 *
 * Supported: drones_per_env == 1; GPD_TASK_NONE and GPD_TASK_HOVER; GPD_ACT_RPM, ONE_D_RPM, RAW_RPM and DIRECT_RPM; physics_flags 0
 * or GPD_PHYS_DRAG; all three airframes; auto_reset == 0.  Everything else (the DSLPID action types, the other flags, D > 1,
 * auto_reset, state.dw_force) returns GPD_ENOTSUP with a message that names the entry and the reason, before any device work.
 */
int gpd_rollout_tape_floats(const GpdStepCfg* cfg, int32_t num_steps, int64_t ld, int64_t* floats_out);
int gpd_rollout_tape(const GpdParams* params, const GpdState* state, const GpdStepCfg* cfg, int32_t num_steps, const float* actions,
                     int64_t action_step_stride, const float* target_pos, float* obs12, int64_t obs_step_stride, float* reward,
                     uint8_t* terminated, uint8_t* truncated, int64_t env_step_stride, const float* plant_rows, float* tape, void* stream);
int gpd_rollout_vjp(const GpdParams* params, const GpdStepCfg* cfg, int64_t ld, int32_t num_steps, const float* actions,
                    int64_t action_step_stride, const float* target_pos, const float* plant_rows, const float* tape,
                    const float* g_obs12, int64_t obs_step_stride, const float* g_reward, int64_t env_step_stride, float* g_kin,
                    float* g_actions, void* stream);
int gpd_rollout_vjp_plant(const GpdParams* params, const GpdStepCfg* cfg, int64_t ld, int32_t num_steps, const float* actions,
                          int64_t action_step_stride, const float* target_pos, const float* plant_rows, const float* tape,
                          const float* g_obs12, int64_t obs_step_stride, const float* g_reward, int64_t env_step_stride, float* g_kin,
                          float* g_actions, float* g_plant_rows, void* stream);
int gpd_plant_derive_vjp(const GpdParams* nominal, const float* scales, const float* g_rows, int32_t n, int64_t ld, float* g_scales,
                         void* stream);

/*
 * The differentiable rollout through the DSLPID loop (additions to ABI 9): the three entries above for the action types that close the
 * loop in the kernel -- GPD_ACT_PID, GPD_ACT_VEL, GPD_ACT_ONE_D_PID -- with the nine controller members (GpdState.pid: integral
 * position error | last rpy | integral rpy error) as a differentiable input and output, and the cotangents of the 18 controller gains.
 * Policy gradients for set-point policies, waypoint optimisation with the controller in the loop, tuning the controller by
 * back-propagation through the flight.  The reference has no counterpart.  gpd_rollout_tape / gpd_rollout_vjp keep refusing these
 * action types.
 *
 * gpd_rollout_tape_pid is gpd_rollout for these action types plus a record of what the sweep needs.  Whatever it leaves behind --
 * state, state.pid, last_rpm, step_counter, bad, obs12, reward and flags -- is bit for bit what gpd_rollout leaves on the same inputs
 * (the same load_carry / map_action / env_step / store_carry code).  The tape is opaque, 16-byte aligned,
 * gpd_rollout_tape_pid_floats(cfg, num_steps, state.ld) floats: the 13 kinematic floats and the nine members every env step starts
 * from, 22 floats = 88 B per drone-step.  The cached roll / pitch / yaw the controller reads are not taped: they are the Euler
 * extraction of the step's start quaternion in every kernel, and the sweep recomputes them with the same instructions.
 *
 * gpd_rollout_vjp_pid is the vector-Jacobian product of (kin_0, pid_0, a_0 .. a_K-1, the 18 gains) -> (kin_K, pid_K, obs12_0 ..,
 * reward_0 ..) of that call:
 *   ld, num_steps, actions, action_step_stride, target_pos   what the taped call was given (ld = state.ld)
 *   g_obs12, g_reward   cotangents of the outputs, laid out like them; NULL = zeros
 *   g_kin               [13*ld], the four-plane layout of GpdState.kin, IN PLACE: the final state's cotangent on entry, the initial
 *                       state's on return.  16-byte aligned
 *   g_pid               [9][ld], the rows of GpdState.pid, IN PLACE in the same way.  16-byte aligned
 *   g_actions           [K][N][A] out (A = 3, 4, 1), ALWAYS one block per step, also for a shared action block.  16-byte aligned for
 *                       GPD_ACT_VEL (its rows are stored as float4)
 *   g_gains             NULL, or [18][ld] out, 16-byte aligned, drones 0 .. N-1 of every row overwritten: PER DRONE, the cotangents of
 *                       p_for[3] | i_for[3] | d_for[3] | p_tor[3] | i_tor[3] | d_tor[3] of GpdParams, summed over the steps in
 *                       registers and stored once after the loop (the forward's gains are shared: the caller sums over drones).
 *                       g_kin, g_pid and g_actions do not depend by a bit on whether it is given
 * One lane per drone, steps K-1 .. 0, the 13 + 9 cotangents in registers; the sub-steps are undone as in gpd_rollout_vjp.  No atomics:
 * two calls give the same bits.  The adjoint is that of the function as executed -- a select differentiates the branch taken, a clamp
 * passes its cotangent on lo <= x <= hi and nothing outside:
 *   the target mappings   PID: inside the 1 m approach limit the target is the action, outside it p + d/|d| (Jacobian (I - dd^T)/|d|
 *                         towards the action, I minus that towards the position); VEL: speed_limit |a_w| a_xyz/|a_xyz| (exactly zero
 *                         at a_xyz = 0), target yaw = the current yaw; ONE_D_PID: 0.1 a + p_z
 *   the position loop     the errors, the three integrators with their clamps (z nested), max(0, .) of the thrust along body z with
 *                         the square root's derivative selected to 0 there, the two normalisations, the cross products, sincos(yaw)
 *   the attitude loop     e_R of R(q) and R*, the finite difference of the Euler angles (it reaches this step's rpy and the last
 *                         rpy, i.e. the previous step), the rate integrators with their clamps, the +-3200 torque clamps, the mixer,
 *                         the PWM clamp, pwm -> rpm, the rotor thrusts
 *   R(q) and rpy(q)       of the step's start state, into the quaternion's cotangent
 * Targets of the task, the mixer, the PWM constants and the target rpy and rates are constants of the sweep.
 *
 * Supported: drones_per_env == 1; the three DSLPID action types; CF2X and CF2P; GPD_TASK_NONE and GPD_TASK_HOVER; physics_flags == 0;
 * auto_reset == 0; no plant table.  GPD_ENOTSUP, before any device work and with a message that names the entry and the reason: the RPM
 * action types (gpd_rollout_tape / gpd_rollout_vjp serve them), any physics flag (drag included), D > 1, GPD_TASK_MULTIHOVER,
 * auto_reset, state.dw_force, an airframe without DSLPID (pid_kf <= 0).  GPD_EINVAL: NULL pointers, a missing state.pid, misaligned
 * kin / g_kin / g_pid / g_gains / tape (and g_actions under GPD_ACT_VEL), bad strides or sizes.  GPD_ERANGE: more than 2^26 drones.
 */
int gpd_rollout_tape_pid_floats(const GpdStepCfg* cfg, int32_t num_steps, int64_t ld, int64_t* floats_out);
int gpd_rollout_tape_pid(const GpdParams* params, const GpdState* state, const GpdStepCfg* cfg, int32_t num_steps, const float* actions,
                         int64_t action_step_stride, const float* target_pos, float* obs12, int64_t obs_step_stride, float* reward,
                         uint8_t* terminated, uint8_t* truncated, int64_t env_step_stride, float* tape, void* stream);
int gpd_rollout_vjp_pid(const GpdParams* params, const GpdStepCfg* cfg, int64_t ld, int32_t num_steps, const float* actions,
                        int64_t action_step_stride, const float* target_pos, const float* tape, const float* g_obs12,
                        int64_t obs_step_stride, const float* g_reward, int64_t env_step_stride, float* g_kin, float* g_pid,
                        float* g_actions, float* g_gains, void* stream);

/*
 * The differentiable rollout through the thrust-and-body-rate loop (additions to ABI 9): the three entries of the differentiable rollout
 * for gpd_rollout_ctbr's flight -- a body-rate loop closed inside every physics sub-step, the command or the target row as the
 * differentiable action -- and the cotangents of the controller's 12 gains.  Policy gradients through the physics on thrust and
 * body-rate actions.  The reference has no counterpart.
 *
 * gpd_rollout_tape_ctbr is gpd_rollout_ctbr (its arguments, in its order) plus a record of what the sweep needs.  Whatever it leaves
 * behind -- state, last_rpm, step_counter, bad, obs12, cmd_out -- is bit for bit what gpd_rollout_ctbr leaves on the same inputs (the same
 * load_carry / gpd_ctbr_outer / gpd_ctbr_rate_loop / substep / store_carry code).  The tape is opaque, 16-byte aligned,
 * gpd_rollout_tape_ctbr_floats(cfg, num_steps, state.ld) = 13 * num_steps * ld floats: the 13 kinematic floats every control step starts
 * from, 52 B per drone-step.  obs_step_stride 0 keeps the last step's rows only, as in gpd_rollout_ctbr.
 *
 * gpd_rollout_vjp_ctbr is the vector-Jacobian product of (kin_0, row_0 .. row_K-1, the 12 gains) -> (kin_K, obs12_0 ..) of that call:
 *   ctbr, ld, mode, num_steps, rows, row_step_stride, plant_rows   what the taped call was given (ld = state.ld).  plant_rows is a
 *                       constant of the sweep: the plant scales receive no gradient here
 *   g_obs12             cotangents of obs12, laid out like it (stride 0: the last step's rows only); NULL = zeros.  16-byte aligned
 *   g_kin               [13*ld], the four-plane layout of GpdState.kin, IN PLACE: the final state's cotangent on entry, the initial
 *                       state's on return.  16-byte aligned
 *   g_rows              [K][N][4] (GPD_CTBR_CMD) or [K][N][12] (GPD_CTBR_POS) out, 16-byte aligned, ALWAYS one block per step, also for a
 *                       held row block (stride 0: the caller sums over the steps).  In GPD_CTBR_POS the rpy and rpy-rate slots of a row
 *                       (floats 3 .. 5 and 9 .. 11), which the forward ignores, receive exact zeros
 *   g_gains             NULL, or [12][ld] out, 16-byte aligned, drones 0 .. N-1 of every row overwritten: PER DRONE, the cotangents of
 *                       k_p[3] | k_d[3] | k_rates[3] | k_rate[3] of GpdCtbr, summed over the steps in registers and stored once after the
 *                       loop (the caller sums over drones).  In GPD_CTBR_CMD the first nine rows are zeros.  g_kin and g_rows do not
 *                       depend by a bit on whether it is given
 * One lane per drone, steps K-1 .. 0, the 13 cotangents in registers.  The RPMs change every sub-step, so sub-step j's start state is
 * recomputed by j x (rate loop, sub-step) from the taped state: S(S+1)/2 of each per control step, no scratch memory, no per-sub-step
 * tape.  No atomics: two calls give the same bits.  The adjoint is that of the function as executed (csrc/ctbr_vjp.inc): the thrust clip,
 * the three rate clips and the per-rotor clip [0, f_max] pass their cotangent on lo <= x <= hi and exactly nothing outside; the chain
 * rotor thrust -> RPM -> thrust deviation is one map with the derivative KF_plant / KF_nominal, so a rotor held at 0 never divides by its
 * RPM; Shepperd's four cases and the q_e.w < 0 negation of the outer loop differentiate the branch taken; the three normalisations are
 * differentiated as 1 / sqrt.  The clips, the allocation, g and the nominal M and J are constants of the sweep.
 *
 * Supported: what gpd_rollout_ctbr serves, with physics_flags == 0.  GPD_ENOTSUP, before any device work and with a message that names
 * the entry and the reason: drones_per_env != 1, a task or auto_reset, an act_type other than GPD_ACT_RAW_RPM / GPD_ACT_DIRECT_RPM, ANY
 * physics flag (drag's rpm sum has an infinite derivative where a rotor is held at 0; ground effect, the ground plane and damping are
 * not differentiated anywhere), state.dw_force.  GPD_EINVAL: NULL pointers (plant_rows, cmd_out, g_obs12, g_gains excepted), an unknown
 * mode or physics flag, misaligned kin / rows / obs12 / plant_rows / cmd_out / tape / g_obs12 / g_kin / g_rows / g_gains, bad strides
 * or sizes, cmd_out == rows, g_rows / g_gains / g_kin / tape overlapping one another.  GPD_ERANGE: more than 2^26 drones.
 */
int gpd_rollout_tape_ctbr_floats(const GpdStepCfg* cfg, int32_t num_steps, int64_t ld, int64_t* floats_out);
int gpd_rollout_tape_ctbr(const GpdParams* params, const GpdCtbr* ctbr, const GpdState* state, const GpdStepCfg* cfg, int32_t mode,
                          const float* rows, int64_t row_step_stride, const float* plant_rows, float* obs12, int64_t obs_step_stride,
                          float* cmd_out, int32_t num_steps, float* tape, void* stream);
int gpd_rollout_vjp_ctbr(const GpdParams* params, const GpdCtbr* ctbr, const GpdStepCfg* cfg, int64_t ld, int32_t mode, int32_t num_steps,
                         const float* rows, int64_t row_step_stride, const float* plant_rows, const float* tape, const float* g_obs12,
                         int64_t obs_step_stride, float* g_kin, float* g_rows, float* g_gains, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* GPD_H */
