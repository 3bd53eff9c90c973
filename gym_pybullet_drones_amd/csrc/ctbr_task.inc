// ctbr_task.inc -- thrust and body-rate commands as a task (include/gpd.h): gpd_task_eval, the single-drone task on rows, and
// gpd_rollout_ctbr_task, K env steps of single-drone aviaries whose ACTION is the command -- the rate loop inside the sub-steps, then the
// task's reward and flags, the same-step auto-reset and the terminal row, one launch.  Pulled into abi.hip behind ctbr.inc; the sub-steps
// are ctbr.inc's ctbr_substeps, the task is gpd_common.inc's task_single: neither is restated.  DESIGN.md section 3.23.
//
// One lane per drone, as gpd_rollout_ctbr_kernel: the state is loaded once and stored once, the next step's command row is requested
// before this step's arithmetic.  The env step follows env_step's single-drone branch (gpd_common.inc) statement for statement from
// quat_to_rpy on: what gpd_rollout_ctbr (GPD_CTBR_CMD, K = 1), gpd_task_eval on its rows and a masked gpd_reset give, bit for bit
// (tests/test_gpu_ctbr_task.py).

namespace {

__global__ __launch_bounds__(kBlock) void gpd_task_eval_kernel(const GpdStepCfg C, const float* __restrict__ obs12,
                                                               const int32_t* __restrict__ counter, const float* __restrict__ target_pos,
                                                               float* __restrict__ reward, uint8_t* __restrict__ terminated,
                                                               uint8_t* __restrict__ truncated) {
    const uint32_t n = blockIdx.x * static_cast<uint32_t>(kBlock) + threadIdx.x;
    if (n >= static_cast<uint32_t>(C.num_envs)) return;
    // (GPD_TASK_NONE: the host passes a readable dummy target, the values are not used)
    const float4* o = reinterpret_cast<const float4*>(reinterpret_cast<const char*>(obs12) + n * 48u);
    const float4 a = o[0], b = o[1];                           // pos | roll, pitch ..
    const float* tp = reinterpret_cast<const float*>(reinterpret_cast<const char*>(target_pos) + (C.target_per_env ? n * 12u : 0u));
    float r;
    bool te, tr;
    task_single(C, a.x, a.y, a.z, a.w, b.x, counter[n], tp[0], tp[1], tp[2], r, te, tr);
    const bool has_task = C.task != GPD_TASK_NONE;
    reward[n] = has_task ? r : -1.0f;
    terminated[n] = static_cast<uint8_t>((has_task & te) ? 1 : 0);
    truncated[n] = static_cast<uint8_t>((has_task & tr) ? 1 : 0);
}

// EXT: any physics flag (tested at run time, uniformly); PLANT: a per-drone plant table.  The action map (`normalized`), the terminal rows
// and cmd_out are wave-uniform branches.  GpdCtbrTask's eight floats travel as two float4, S4 (scale) and O4 (bias), next to the three
// structs: the argument segment holds no array the compiler would index through scratch.
template <bool EXT, bool PLANT>
__global__ __launch_bounds__(kBlock) void ctbr_task_kernel(
    const GpdParams P, const GpdCtbr B, float* __restrict__ kin, float* __restrict__ last_rpm, int32_t* __restrict__ step_counter,
    uint8_t* __restrict__ bad, const uint32_t ld32, const GpdStepCfg C, const float4 S4, const float4 O4, const int normalized,
    const float* __restrict__ actions, const int64_t astride, const float* __restrict__ target_pos, const float* __restrict__ init_pose,
    const float* __restrict__ plant, float* __restrict__ obs12, float* __restrict__ term_obs12, const int64_t ostride,
    float* __restrict__ reward, uint8_t* __restrict__ terminated, uint8_t* __restrict__ truncated, const int64_t estride,
    float* __restrict__ cmd_out, const int K) {
    const uint32_t n = blockIdx.x * static_cast<uint32_t>(kBlock) + threadIdx.x;
    if (n >= static_cast<uint32_t>(C.num_envs)) return;
    const GpdState S{kin, last_rpm, nullptr, step_counter, static_cast<int64_t>(ld32), nullptr, nullptr, nullptr, 0, 0, bad};
    const uint32_t flags = EXT ? C.physics_flags : 0u;
    Lane L;
    L.n = n; L.env = n; L.tid = threadIdx.x; L.le = threadIdx.x; L.d = 0; L.base = threadIdx.x; L.active = true; L.shfl = false;
    Carry c;
    float tgx, tgy, tgz, ip[7];
    // (no auto-reset: the reset pose is never used; the host hands state.kin as init_pose with init_per_env = 0, so every lane reads
    // the first seven floats of kin -- readable, cached, ignored)
    const float* ipose = reinterpret_cast<const float*>(reinterpret_cast<const char*>(init_pose) + (C.init_per_env ? n * 28u : 0u));
    load_carry<false, EXT>(S, C, flags, L, target_pos, C.auto_reset ? ipose : kin, c, tgx, tgy, tgz, ip);
    // the reset pose's Euler angles, once per launch: the bits gpd_reset writes
    float irpy[3] = {0.0f, 0.0f, 0.0f};
    if (C.auto_reset) quat_to_rpy(ip[3], ip[4], ip[5], ip[6], irpy[0], irpy[1], irpy[2]);
    plant_t<PLANT> Q = plant_of<PLANT>(P, plant, S.ld, n * 4u);
    Kin& k = c.k;
    const bool drag = EXT && (flags & GPD_PHYS_DRAG);
    const bool has_task = C.task != GPD_TASK_NONE;
    float avx = 0.0f, avy = 0.0f, avz = 0.0f;
    float4 act = load_action<4>(actions, n);
    for (int t = 0; t < K; ++t) {
        // the NEXT step's row is requested before this step's arithmetic (a held row -- stride 0 -- is read again, a cache hit)
        const float4 nx = load_action<4>(actions + (t + 1 < K ? t + 1 : t) * astride, n);
        // ---- the command: the action as it is, or its affine map
        float cmd[4] = {act.x, act.y, act.z, act.w};
        if (normalized) {
            cmd[0] = fmaf(act.x, S4.x, O4.x); cmd[1] = fmaf(act.y, S4.y, O4.y); cmd[2] = fmaf(act.z, S4.z, O4.z); cmd[3] = fmaf(act.w, S4.w, O4.w);
        }
        if (cmd_out) *reinterpret_cast<float4*>(reinterpret_cast<char*>(cmd_out + t * astride) + n * 16u) = make_float4(cmd[0], cmd[1], cmd[2], cmd[3]);
        // ---- S sub-steps, the rate loop in each; the rpy refresh
        ctbr_substeps<EXT>(P, B, Q, C, flags, drag, cmd, c, avx, avy, avz);
        quat_to_rpy(k.qx, k.qy, k.qz, k.qw, c.roll, c.pitch, c.yaw);
        // ---- the task, masked by the (uniform) task switch, on the counter before the increment
        float r;
        bool te, tr;
        task_single(C, k.px, k.py, k.pz, c.roll, c.pitch, c.counter, tgx, tgy, tgz, r, te, tr);
        const float rew = has_task ? r : -1.0f;
        const bool term = has_task & te, trunc = has_task & tr;
        const bool do_reset = C.auto_reset && (term || trunc);
        c.counter = do_reset ? 0 : c.counter + C.substeps;
        // ---- same-step auto-reset, as env_step does it
        if (any_lane(do_reset)) {
            asm volatile("; episode end");
            if (do_reset) {
                if (term_obs12 && (ostride != 0 || t == K - 1)) store_obs12(term_obs12 + t * ostride, n, k.px, k.py, k.pz, c.roll, c.pitch, c.yaw, k.vx, k.vy, k.vz, avx, avy, avz);
                k = Kin{ip[0], ip[1], ip[2], ip[3], ip[4], ip[5], ip[6], 0, 0, 0, 0, 0, 0};
                c.roll = irpy[0]; c.pitch = irpy[1]; c.yaw = irpy[2];
                avx = avy = avz = 0.0f;
                c.l0 = c.l1 = c.l2 = c.l3 = 0.0f;
            }
        }
        // ---- the row of the state the step leaves, the aviary's outputs
        if (ostride != 0 || t == K - 1) store_obs12(obs12 + t * ostride, n, k.px, k.py, k.pz, c.roll, c.pitch, c.yaw, k.vx, k.vy, k.vz, avx, avy, avz);
        if (estride != 0 || t == K - 1) {
            const int64_t at = t * estride + n;
            reward[at] = rew;
            terminated[at] = static_cast<uint8_t>(term ? 1 : 0);
            truncated[at] = static_cast<uint8_t>(trunc ? 1 : 0);
        }
        act = nx;
    }
    store_carry<false>(S, L, c);
}

}  // namespace

extern "C" int gpd_sizeof_ctbr_task(int32_t* size_out) {
    if (!size_out) return Refuse{"gpd_sizeof_ctbr_task"}(GPD_EINVAL, "NULL size_out");
    *size_out = static_cast<int32_t>(sizeof(GpdCtbrTask));
    return 0;
}

extern "C" int gpd_task_eval(const GpdStepCfg* cfg, const float* obs12, const int32_t* counter, const float* target_pos, float* reward,
                             uint8_t* terminated, uint8_t* truncated, void* stream) {
    const Refuse bad{"gpd_task_eval"};
    if (!cfg || !obs12 || !counter || !reward || !terminated || !truncated) return bad(GPD_EINVAL, "NULL cfg/obs12/counter/reward/terminated/truncated");
    if (cfg->num_envs <= 0) return bad(GPD_EINVAL, "num_envs must be positive");
    if (cfg->task < GPD_TASK_NONE || cfg->task > GPD_TASK_MULTIHOVER) return bad(GPD_EINVAL, "unknown task");
    if (cfg->drones_per_env != 1) return bad(GPD_ENOTSUP, "aviaries of one drone only");
    if (cfg->task == GPD_TASK_MULTIHOVER) return bad(GPD_ENOTSUP, "task must be GPD_TASK_NONE or GPD_TASK_HOVER");
    if (cfg->num_envs > (1 << 26)) return bad(GPD_ERANGE, "more than 2^26 drones per launch (32-bit byte offsets)");
    if (cfg->task != GPD_TASK_NONE && !target_pos) return bad(GPD_EINVAL, "task needs target_pos");
    if (misaligned16(obs12)) return bad(GPD_EINVAL, "obs12 must be 16-byte aligned");
    GpdStepCfg c = *cfg;
    dummy_target(c, target_pos, obs12);
    hipLaunchKernelGGL(gpd_task_eval_kernel, dim3(blocks_for(c.num_envs, kBlock)), dim3(kBlock), 0, static_cast<hipStream_t>(stream), c, obs12, counter,
                       target_pos, reward, terminated, truncated);
    return launched(bad.who);
}

extern "C" int gpd_rollout_ctbr_task(const GpdParams* params, const GpdCtbr* ctbr, const GpdState* state, const GpdStepCfg* cfg,
                                     const GpdCtbrTask* task, int32_t num_steps, const float* actions, int64_t action_step_stride,
                                     const float* target_pos, const float* init_pose, const float* plant_rows, float* obs12,
                                     float* term_obs12, int64_t obs_step_stride, float* reward, uint8_t* terminated, uint8_t* truncated,
                                     int64_t env_step_stride, float* cmd_out, void* stream) {
    const Refuse bad{"gpd_rollout_ctbr_task"};
    if (!params || !ctbr || !state || !cfg) return bad(GPD_EINVAL, "NULL params/ctbr/state/cfg");
    if (int rc = check_state(bad, state)) return rc;
    if (!actions || !obs12 || !reward || !terminated || !truncated) return bad(GPD_EINVAL, "NULL actions/obs12/reward/terminated/truncated");
    if (int rc = check_steps(bad, num_steps, action_step_stride, obs_step_stride, env_step_stride)) return rc;
    if (int rc = check_flags(bad, cfg)) return rc;
    if (cfg->task < GPD_TASK_NONE || cfg->task > GPD_TASK_MULTIHOVER) return bad(GPD_EINVAL, "unknown task");
    // what the kernel serves, in front of the remaining shared checks (a configuration outside it answers GPD_ENOTSUP)
    if (cfg->drones_per_env != 1) return bad(GPD_ENOTSUP, "aviaries of one drone only");
    if (cfg->task == GPD_TASK_MULTIHOVER) return bad(GPD_ENOTSUP, "task must be GPD_TASK_NONE or GPD_TASK_HOVER");
    if (cfg->act_type != GPD_ACT_RAW_RPM && cfg->act_type != GPD_ACT_DIRECT_RPM)
        return bad(GPD_ENOTSUP, "act_type GPD_ACT_RAW_RPM or GPD_ACT_DIRECT_RPM (the rate loop's output is RPMs)");
    if ((cfg->physics_flags & GPD_PHYS_DW) || state->dw_force) return bad(GPD_ENOTSUP, "downwash needs mates");
    if (state->act_ring) return bad(GPD_ENOTSUP, "state.act_ring (the action history) is not served here");
    if (int rc = check_positive(bad, cfg)) return rc;
    const int64_t N = cfg->num_envs;
    if (int rc = check_extent(bad, N, state->ld)) return rc;
    if (int rc = check_needs(bad, params, state, cfg, target_pos, init_pose)) return rc;
    if ((action_step_stride != 0 && action_step_stride < 4 * N) || (obs_step_stride != 0 && obs_step_stride < 12 * N) ||
        (env_step_stride != 0 && env_step_stride < N))
        return bad(GPD_EINVAL, "a non-zero step stride must cover a step's rows (4*num_envs actions, 12*num_envs for obs12, num_envs per aviary output)");
    if ((action_step_stride & 3) || (obs_step_stride & 3)) return bad(GPD_EINVAL, "action and obs step strides must be multiples of 4 floats (16-byte rows)");
    if (misaligned16(actions) || misaligned16(obs12) || misaligned16(term_obs12) || misaligned16(plant_rows) || misaligned16(cmd_out))
        return bad(GPD_EINVAL, "actions, obs12, term_obs12, plant_rows and cmd_out must be 16-byte aligned");
    if (cmd_out && cmd_out == actions) return bad(GPD_EINVAL, "cmd_out must not alias actions");
    if (term_obs12 && term_obs12 == obs12) return bad(GPD_EINVAL, "term_obs12 must not alias obs12");
    if (!(cfg->ctrl_dt > 0.0f) || !(cfg->pyb_dt > 0.0f)) return bad(GPD_EINVAL, "pyb_dt and ctrl_dt must be positive");
    if (task && task->normalized != 0 && task->normalized != 1) return bad(GPD_EINVAL, "task.normalized must be 0 or 1");
    GpdStepCfg C = *cfg;
    C.drones_per_env = 1;
    dummy_target(C, target_pos, state->kin);
    if (!C.auto_reset) { C.init_per_env = 0; init_pose = state->kin; }
    const bool norm = task && task->normalized;
    const float4 s4 = norm ? make_float4(task->act_scale[0], task->act_scale[1], task->act_scale[2], task->act_scale[3]) : make_float4(1.0f, 1.0f, 1.0f, 1.0f);
    const float4 o4 = norm ? make_float4(task->act_bias[0], task->act_bias[1], task->act_bias[2], task->act_bias[3]) : make_float4(0.0f, 0.0f, 0.0f, 0.0f);
    const bool ext = (C.physics_flags & 31u) != 0;
    const dim3 grid(blocks_for(N, kBlock));
    hipStream_t st = static_cast<hipStream_t>(stream);
    with_ext_plant(ext, plant_rows != nullptr, [&](auto ext_, auto plant_) {
        hipLaunchKernelGGL((ctbr_task_kernel<decltype(ext_)::value, decltype(plant_)::value>), grid, dim3(kBlock), 0, st, *params, *ctbr, state->kin,
                           state->last_rpm, state->step_counter, state->bad, static_cast<uint32_t>(state->ld), C, s4, o4, norm ? 1 : 0, actions,
                           action_step_stride, target_pos, init_pose, plant_rows, obs12, term_obs12, obs_step_stride, reward, terminated, truncated,
                           env_step_stride, cmd_out, num_steps);
    });
    return launched(bad.who);
}
