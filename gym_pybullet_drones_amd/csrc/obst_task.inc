// obst_task.inc -- gpd_rollout_obst (include/gpd.h): obstacle courses as a task.  K env steps per launch of single-drone aviaries, and in
// every step the clearance of the pose the step reached (contact ends the episode and is scored), the same-step auto-reset on the
// combined flags, and the observation row  pos rpy vel ang_v | nx ny nz d | ranges  of the pose the step leaves behind.  Pulled into
// abi.hip after obstacles.inc; the combination is obst_task_math.inc, the text a host program compiles too.  DESIGN.md section 3.22.
//
// One kernel, one launch, no atomics, one writer per word.  A GROUP of G lanes per drone, G the smallest power of two >= max(1, n_rays):
//   * every lane of a group carries the drone's state and runs the same physics on it -- group-uniform addresses for the state, action
//     and target loads, identical bits in every lane, no cross-lane traffic;
//   * the clearance walk is split over the group -- lane j takes records j, j + G .. -- and reduced by the lexicographic minimum of
//     (d, record) with __shfl_xor inside the group: a total order, so every lane ends with the sequential strict-`<` answer;
//   * lane j casts ray j (every lane walks the whole list at the same index: a shared list's kind goes through v_readfirstlane, as in
//     obstacles.inc);
//   * the group stores the row together: lanes 0 .. 3 one 16-byte piece each, lane j range j; lane 0 writes the per-aviary outputs and,
//     once per launch, the state.
// The env step follows env_step's single-drone branch (gpd_common.inc) statement for statement -- map_action, the sub-steps in the same
// pairs with the last one's angular velocity, quat_to_rpy, task_single masked by the task -- with the clearance between the task and the
// reset: what gpd_step, gpd_obstacles, a masked gpd_reset and gpd_obstacles again give, bit for bit (tests/test_gpu_obst_task.py).
#include "obst_task_math.inc"

namespace {

// a record for ONE lane (the split clearance walk: the lanes of a wave are at different records, so the kind stays a vector value)
template <bool SHARED>
__device__ __forceinline__ ObstRecord obst_task_record(const float* __restrict__ obst, const float4* lds, int m, int64_t ld, int64_t e) {
    ObstRecord r;
    if constexpr (SHARED) {
        const float4 a = lds[2 * m], b = lds[2 * m + 1];
        r.cx = a.x; r.cy = a.y; r.cz = a.z; r.ax = b.x; r.ay = b.y; r.az = b.z;
        r.kind = obst_kind(a.w);
    } else {
        r = obst_record<false>(obst, lds, m, ld, e);
    }
    return r;
}

// ACT: GPD_ACT_RPM, GPD_ACT_PID or GPD_ACT_VEL; EXT: any physics flag (tested at run time, uniformly); SHARED: one list in LDS
template <int ACT, bool EXT, bool SHARED>
__global__ __launch_bounds__(kBlock) void obst_task_kernel(
    const GpdParams P, const GpdState S, const GpdStepCfg C, const GpdObstTask Q, const int K, const int gshift,
    const float* __restrict__ action, const int64_t action_stride, const float* __restrict__ target_pos, const float* __restrict__ init_pose,
    const float* __restrict__ obst, const int n_obst, const int64_t obst_ld, const float* __restrict__ ray_dirs, float* __restrict__ rows,
    const int64_t row_ld, const int64_t row_stride, float* __restrict__ reward, uint8_t* __restrict__ terminated,
    uint8_t* __restrict__ truncated, uint8_t* __restrict__ collided, const int64_t env_stride) {
    constexpr bool PID = ACT != GPD_ACT_RPM;
    constexpr int AW = ACT == GPD_ACT_PID ? 3 : 4;
    extern __shared__ __attribute__((aligned(16))) float4 obst_lds[];
    obst_stage<SHARED>(obst, n_obst, obst_lds);              // once per workgroup, reused by all K steps
    const int tid = threadIdx.x;
    const int G = 1 << gshift, j = tid & (G - 1);
    const uint32_t N = static_cast<uint32_t>(C.num_envs);
    const uint32_t n_raw = blockIdx.x * static_cast<uint32_t>(kBlock >> gshift) + static_cast<uint32_t>(tid >> gshift);   // (< 2^26 + 256)
    // a group without a drone (ragged last workgroup) computes on drone 0 and stores nothing
    Lane L;
    L.tid = tid; L.active = n_raw < N; L.n = L.active ? n_raw : 0u; L.env = L.n; L.le = tid; L.d = 0; L.base = tid; L.shfl = false;
    const uint32_t flags = EXT ? C.physics_flags : 0u;
    const int R = Q.n_rays;
    const int64_t e = SHARED ? 0 : static_cast<int64_t>(L.n);

    Carry c;
    float tgx, tgy, tgz, ip[7];
    const float* ipose = reinterpret_cast<const float*>(reinterpret_cast<const char*>(init_pose) + (C.init_per_env ? L.n * 28u : 0u));
    load_carry<PID, EXT>(S, C, flags, L, target_pos, C.auto_reset ? ipose : S.kin, c, tgx, tgy, tgz, ip);
    c.roll = c.pitch = c.yaw = 0.0f;
    if (PID) quat_to_rpy(c.k.qx, c.k.qy, c.k.qz, c.k.qw, c.roll, c.pitch, c.yaw);
    float irpy[3] = {0.0f, 0.0f, 0.0f};
    if (C.auto_reset) quat_to_rpy(ip[3], ip[4], ip[5], ip[6], irpy[0], irpy[1], irpy[2]);
    // this lane's ray (lanes past the last ray of a group walk with ray 0 and store nothing)
    float rdx = 1.0f, rdy = 0.0f, rdz = 0.0f;
    if (R > 0) { const int ray = j < R ? j : 0; rdx = ray_dirs[3 * ray]; rdy = ray_dirs[3 * ray + 1]; rdz = ray_dirs[3 * ray + 2]; }

    // the minimum over the records of each one's signed distance, with that record's gradient: (0, 0, 0, +inf) without a live record
    // or a finite position.  Called by every lane of the wave together.
    auto clearance = [&](float px, float py, float pz, float& nx, float& ny, float& nz, float& d) {
        float best = GPD_OBST_INF, bx = 0.0f, by = 0.0f, bz = 0.0f;
        int who = -1;
        if (finite3(px, py, pz)) {
            for (int m = j; m < n_obst; m += G) {
                const ObstRecord r = obst_task_record<SHARED>(obst, obst_lds, m, obst_ld, e);
                float gx, gy, gz;
                const float dm = gpd_obst_sdf(r.kind, r.ax, r.ay, r.az, px - r.cx, py - r.cy, pz - r.cz, &gx, &gy, &gz);
                const bool closer = dm < best;           // (strict: a tie keeps the lower m; false for a NaN)
                best = closer ? dm : best;
                bx = closer ? gx : bx; by = closer ? gy : by; bz = closer ? gz : bz;
                who = closer ? m : who;
            }
        }
        for (int w = 1; w < G; w <<= 1) {                // (best is never a NaN, who is -1 exactly where best is +inf: a total order)
            const float od = __shfl_xor(best, w), ox = __shfl_xor(bx, w), oy = __shfl_xor(by, w), oz = __shfl_xor(bz, w);
            const int ow = __shfl_xor(who, w);
            const bool take = (od < best) | ((od == best) & (ow < who));
            best = take ? od : best;
            bx = take ? ox : bx; by = take ? oy : by; bz = take ? oz : bz;
            who = take ? ow : who;
        }
        nx = bx; ny = by; nz = bz; d = best;
    };
    // this lane's ray from the pose (p, q): the smallest entry over the records, capped at max_range
    auto scan = [&](float px, float py, float pz, float qx, float qy, float qz, float qw) {
        float dx = rdx, dy = rdy, dz = rdz;
        if (Q.ray_frame != GPD_RAY_WORLD) obst_turn_ray(Q.ray_frame, qx, qy, qz, qw, dx, dy, dz);      // (wave-uniform)
        float best = Q.max_range;
        if (finite3(px, py, pz) && finite3(dx, dy, dz)) {
            for (int m = 0; m < n_obst; ++m) {
                const ObstRecord r = obst_record<SHARED>(obst, obst_lds, m, obst_ld, e);
                const float t = gpd_obst_ray(r.kind, r.ax, r.ay, r.az, px - r.cx, py - r.cy, pz - r.cz, dx, dy, dz);
                best = t < best ? t : best;              // (strict: an entry AT max_range is no hit)
            }
        }
        return best;
    };

    auto fetch = [&](int step) { return load_action<AW>(action + (step < K ? step : K - 1) * action_stride, L.n); };
    auto do_step = [&](const int t, const float4 act) {
        Kin& k = c.k;
        float rpm[4], g[4];
        map_action<PID, AW, ACT>(P, C, act, c, rpm, g);
        // ---- the sub-steps, as env_step pairs them; only the last one's world angular velocity is observed ----
        const float cur_sum = ((rpm[0] + rpm[1]) + rpm[2]) + rpm[3];
        float drag_sum = (EXT && (flags & GPD_PHYS_DRAG)) ? ((c.l0 + c.l1) + c.l2) + c.l3 : cur_sum;
        float avx = 0.0f, avy = 0.0f, avz = 0.0f;
        {
            const float dw = EXT ? c.dw_in : 0.0f;
            int left = C.substeps;
            for (; left > 2; left -= 2) {
                substep<EXT, false>(P, C.pyb_dt, flags, g, drag_sum, dw, k, avx, avy, avz);
                substep<EXT, false>(P, C.pyb_dt, flags, g, cur_sum, dw, k, avx, avy, avz);
                drag_sum = cur_sum;
            }
            if (left == 2) {
                substep<EXT, false>(P, C.pyb_dt, flags, g, drag_sum, dw, k, avx, avy, avz);
                drag_sum = cur_sum;
            }
            substep<EXT, true>(P, C.pyb_dt, flags, g, drag_sum, dw, k, avx, avy, avz);
        }
        quat_to_rpy(k.qx, k.qy, k.qz, k.qw, c.roll, c.pitch, c.yaw);
        // ---- the task, masked by the (uniform) task switch ----
        float tr_;
        bool te, tr;
        task_single(C, k.px, k.py, k.pz, c.roll, c.pitch, c.counter, tgx, tgy, tgz, tr_, te, tr);
        const bool has_task = C.task != GPD_TASK_NONE;
        float rew = has_task ? tr_ : -1.0f;
        bool term = has_task & te;
        const bool trunc = has_task & tr;
        // ---- clearance of the pose the step reached; contact ----
        float nx, ny, nz, d;
        clearance(k.px, k.py, k.pz, nx, ny, nz, d);
        const bool hit = gpd_obst_task_hit(d, Q.collision_radius) != 0;
        rew = gpd_obst_task_reward(rew, d, Q.collision_radius, Q.hit_reward, Q.prox_margin, Q.prox_weight);
        term = term | ((Q.hit_terminates != 0) & hit);
        // ---- same-step auto-reset on the combined flags, as env_step does it ----
        const bool do_reset = C.auto_reset && (term || trunc);
        c.counter = do_reset ? 0 : c.counter + C.substeps;
        c.l0 = rpm[0]; c.l1 = rpm[1]; c.l2 = rpm[2]; c.l3 = rpm[3];
        if (any_lane(do_reset)) {
            asm volatile("; episode end");
            if (do_reset) {
                k = Kin{ip[0], ip[1], ip[2], ip[3], ip[4], ip[5], ip[6], 0, 0, 0, 0, 0, 0};
                c.roll = irpy[0]; c.pitch = irpy[1]; c.yaw = irpy[2];
                avx = avy = avz = 0.0f;
                c.l0 = c.l1 = c.l2 = c.l3 = 0.0f;
            }
            // the row shows the clearance of the pose that is observed: the whole wave walks again (a group resets as one, its lanes
            // shuffle among themselves), the groups that kept their pose keep their values
            float rx, ry, rz, rd;
            clearance(k.px, k.py, k.pz, rx, ry, rz, rd);
            nx = do_reset ? rx : nx; ny = do_reset ? ry : ny; nz = do_reset ? rz : nz; d = do_reset ? rd : d;
        }
        float range = 0.0f;
        if (R > 0) range = scan(k.px, k.py, k.pz, k.qx, k.qy, k.qz, k.qw);
        // ---- the row, the aviary's outputs ----
        if (L.active) {
            float* row = rows + t * row_stride + static_cast<int64_t>(L.n) * row_ld;
            for (int ch = j; ch < 4; ch += G) {
                const f4v v = ch == 0 ? f4v{k.px, k.py, k.pz, c.roll} : ch == 1 ? f4v{c.pitch, c.yaw, k.vx, k.vy}
                            : ch == 2 ? f4v{k.vz, avx, avy, avz} : f4v{nx, ny, nz, d};
                __builtin_nontemporal_store(v, reinterpret_cast<f4v*>(row) + ch);
            }
            if (j < R) __builtin_nontemporal_store(range, row + 16 + j);
            if (j == 0) {
                const int64_t at = t * env_stride + static_cast<int64_t>(L.env);
                __builtin_nontemporal_store(rew, reward + at);
                __builtin_nontemporal_store(static_cast<uint8_t>(term ? 1 : 0), terminated + at);
                __builtin_nontemporal_store(static_cast<uint8_t>(trunc ? 1 : 0), truncated + at);
                __builtin_nontemporal_store(static_cast<uint8_t>(hit ? 1 : 0), collided + at);
            }
        }
    };
    float4 act = fetch(0);
    for (int t = 0; t < K; ++t) {
        const float4 act_next = fetch(t + 1);            // (one step of look-ahead: the row arrives within the step)
        do_step(t, act);
        act = act_next;
    }
    if (L.active && j == 0) store_carry<PID>(S, L, c);
}

inline bool obst_task_finite(float v) { return fabsf(v) < GPD_OBST_INF; }      // (false for NaN)

}  // namespace

extern "C" int gpd_sizeof_obst_task(int32_t* size_out) {
    if (!size_out) return Refuse{"gpd_sizeof_obst_task"}(GPD_EINVAL, "NULL size_out");
    *size_out = static_cast<int32_t>(sizeof(GpdObstTask));
    return 0;
}

extern "C" int gpd_rollout_obst(const GpdParams* params, const GpdState* state, const GpdStepCfg* cfg, const GpdObstTask* task,
                                int32_t num_steps, const float* actions, int64_t action_step_stride, const float* target_pos,
                                const float* init_pose, const float* obst, int32_t n_obst, int64_t obst_ld, const float* ray_dirs, float* rows,
                                int64_t row_ld, int64_t row_step_stride, float* reward, uint8_t* terminated, uint8_t* truncated,
                                uint8_t* collided, int64_t env_step_stride, void* stream) {
    const Refuse bad{"gpd_rollout_obst"};
    if (int rc = check_steps(bad, num_steps, action_step_stride, row_step_stride, env_step_stride)) return rc;
    if (!params || !state || !cfg || !task) return bad(GPD_EINVAL, "NULL params/state/cfg/task");
    if (int rc = check_state(bad, state)) return rc;
    if (!actions || !obst || !rows || !reward || !terminated || !truncated || !collided)
        return bad(GPD_EINVAL, "NULL actions/obst/rows/reward/terminated/truncated/collided");
    if (int rc = check_positive(bad, cfg)) return rc;
    if (int rc = check_ranges(bad, cfg)) return rc;
    if (int rc = check_flags(bad, cfg)) return rc;
    // what narrows this entry
    if (cfg->drones_per_env != 1) return bad(GPD_ENOTSUP, "drones_per_env must be 1 (an obstacle course is flown by single drones)");
    if (cfg->act_type != GPD_ACT_RPM && cfg->act_type != GPD_ACT_VEL && cfg->act_type != GPD_ACT_PID)
        return bad(GPD_ENOTSUP, "act_type must be GPD_ACT_RPM, GPD_ACT_VEL or GPD_ACT_PID");
    if (cfg->task == GPD_TASK_MULTIHOVER) return bad(GPD_ENOTSUP, "task must be GPD_TASK_NONE or GPD_TASK_HOVER");
    if (cfg->physics_flags & GPD_PHYS_DW) return bad(GPD_ENOTSUP, "GPD_PHYS_DW: downwash needs mates, the course is flown alone");
    if (state->bad) return bad(GPD_ENOTSUP, "state.bad (the non-finite guard) is not served here");
    if (state->act_ring) return bad(GPD_ENOTSUP, "state.act_ring (the action history) is not served here");
    const int64_t N = cfg->num_envs;
    if (int rc = check_extent(bad, N, state->ld)) return rc;
    if (int rc = check_needs(bad, params, state, cfg, target_pos, init_pose)) return rc;
    // the obstacle list, as gpd_obstacles takes it
    if (n_obst < 1 || n_obst > GPD_OBST_MAX) return bad(GPD_ERANGE, "n_obst must be in 1..1024");
    const bool shared = obst_ld == 1;
    if (!shared && obst_ld < N) return bad(GPD_EINVAL, "obst_ld must be 1 (one shared list) or >= num_envs (one list per aviary)");
    // the task
    if (!(task->collision_radius > 0.0f) || !obst_task_finite(task->collision_radius))
        return bad(GPD_EINVAL, "collision_radius must be positive and finite");
    if (task->hit_terminates != 0 && task->hit_terminates != 1) return bad(GPD_EINVAL, "hit_terminates must be 0 or 1");
    if (!obst_task_finite(task->hit_reward)) return bad(GPD_EINVAL, "hit_reward must be finite");
    if (!(task->prox_margin >= 0.0f) || !obst_task_finite(task->prox_margin) || !(task->prox_weight >= 0.0f) || !obst_task_finite(task->prox_weight))
        return bad(GPD_EINVAL, "prox_margin and prox_weight must be non-negative and finite");
    if (task->n_rays < 0 || task->n_rays > GPD_OBST_MAX_RAYS) return bad(GPD_ERANGE, "n_rays must be in 0..64");
    if (task->n_rays > 0) {
        if (!ray_dirs) return bad(GPD_EINVAL, "n_rays > 0 needs ray_dirs");
        if (task->ray_frame < GPD_RAY_WORLD || task->ray_frame > GPD_RAY_BODY) return bad(GPD_EINVAL, "unknown ray_frame");
        if (!(task->max_range > 0.0f) || !obst_task_finite(task->max_range)) return bad(GPD_EINVAL, "max_range must be positive and finite");
    }
    // the rows
    if (misaligned16(rows)) return bad(GPD_EINVAL, "rows must be 16-byte aligned");
    if (row_ld % 4 != 0 || row_ld < 16 + task->n_rays) return bad(GPD_EINVAL, "row_ld must be a multiple of 4 and >= 16 + n_rays");
    if (row_step_stride % 4 != 0) return bad(GPD_EINVAL, "row_step_stride must be a multiple of 4 (the rows are stored as 16-byte pieces)");

    GpdStepCfg c = *cfg;
    dummy_target(c, target_pos, state->kin);
    GpdObstTask q = *task;
    if (q.n_rays == 0) { q.ray_frame = GPD_RAY_WORLD; q.max_range = 1.0f; }
    int gshift = 0;
    while ((1 << gshift) < q.n_rays) ++gshift;               // G = 1 << gshift: the smallest power of two >= max(1, n_rays)
    const unsigned grid = blocks_for(N, kBlock >> gshift);   // (<= 2^26 / 4 workgroups)
    const size_t lds = shared ? static_cast<size_t>(n_obst) * GPD_OBST_FLOATS * sizeof(float) : 0;
    hipStream_t st = static_cast<hipStream_t>(stream);
    auto go = [&](auto act, auto ext, auto sh) {
        hipLaunchKernelGGL((obst_task_kernel<decltype(act)::value, decltype(ext)::value, decltype(sh)::value>), dim3(grid), dim3(kBlock), lds, st,
                           *params, *state, c, q, num_steps, gshift, actions, action_step_stride, target_pos, init_pose, obst, n_obst, obst_ld,
                           ray_dirs, rows, row_ld, row_step_stride, reward, terminated, truncated, collided, env_step_stride);
    };
    auto with_act = [&](auto act) {
        if (cfg->physics_flags != 0) { if (shared) go(act, Const<true>{}, Const<true>{}); else go(act, Const<true>{}, Const<false>{}); }
        else { if (shared) go(act, Const<false>{}, Const<true>{}); else go(act, Const<false>{}, Const<false>{}); }
    };
    switch (cfg->act_type) {
        case GPD_ACT_PID: with_act(Const<static_cast<int>(GPD_ACT_PID)>{}); break;
        case GPD_ACT_VEL: with_act(Const<static_cast<int>(GPD_ACT_VEL)>{}); break;
        default: with_act(Const<static_cast<int>(GPD_ACT_RPM)>{}); break;
    }
    return launched(bad.who);
}
