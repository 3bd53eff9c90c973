// ctbr.inc -- thrust and body-rate commands (include/gpd.h): the batched outer loop of the reference's CTBRControl (gpd_ctbr) and the
// K-step rollout that closes a body-rate loop inside the physics sub-steps (gpd_rollout_ctbr).  Pulled into abi.hip; the arithmetic of
// both loops is ctbr_math.inc, the text a host program compiles too.  DESIGN.md section 3.17.
//
// One lane per drone.  The controller carries no state but the last RPMs (the drag term's "previous action"), so next to the physics a
// lane holds the command (4 VGPRs) and, in GPD_CTBR_POS, the prefetched target row; GpdCtbr is 32 wave-uniform floats in SGPRs.
#include "ctbr_math.inc"

namespace {

__global__ __launch_bounds__(kBlock) void gpd_ctbr_kernel(const GpdCtbr B, const float* __restrict__ cur_pos, const float* __restrict__ cur_quat,
                                                          const float* __restrict__ cur_vel, const float* __restrict__ target_pos,
                                                          const float* __restrict__ target_vel, float* __restrict__ cmd_out, const int n_total) {
    const uint32_t n = blockIdx.x * static_cast<uint32_t>(kBlock) + threadIdx.x;
    if (n >= static_cast<uint32_t>(n_total)) return;
    const uint32_t n3 = n * 3u;
    const float4 q = reinterpret_cast<const float4*>(cur_quat)[n];
    float tvx = 0.0f, tvy = 0.0f, tvz = 0.0f;
    if (target_vel) { tvx = target_vel[n3]; tvy = target_vel[n3 + 1]; tvz = target_vel[n3 + 2]; }
    float cmd[4];
    gpd_ctbr_outer(&B, cur_pos[n3], cur_pos[n3 + 1], cur_pos[n3 + 2], q.x, q.y, q.z, q.w, cur_vel[n3], cur_vel[n3 + 1], cur_vel[n3 + 2],
                   target_pos[n3], target_pos[n3 + 1], target_pos[n3 + 2], tvx, tvy, tvz, cmd);
    reinterpret_cast<float4*>(cmd_out)[n] = make_float4(cmd[0], cmd[1], cmd[2], cmd[3]);
}

// the rows of one drone at one step: a command (the first 16 bytes) or a target row (48 bytes)
struct CtbrRow { float4 a, b, c; };
template <int MODE>
__device__ __forceinline__ CtbrRow ctbr_row(const float* __restrict__ rows, uint32_t n) {
    if constexpr (MODE == GPD_CTBR_POS) {
        const float4* p = reinterpret_cast<const float4*>(reinterpret_cast<const char*>(rows) + n * 48u);
        return CtbrRow{p[0], p[1], p[2]};
    } else {
        const float4 z = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
        return CtbrRow{*reinterpret_cast<const float4*>(reinterpret_cast<const char*>(rows) + n * 16u), z, z};
    }
}

// One physics sub-step under the rate loop, for gpd_rollout_ctbr_kernel and ctbr_task_kernel (ctbr_task.inc) alike: the command is held,
// the body rates are the integrator's own, and the drag term sees the RPMs applied one sub-step earlier (state.last_rpm on the launch's
// very first one).  AV: this sub-step's world angular velocity is observed.
template <bool EXT, bool AV, class PL>
__device__ __forceinline__ void ctbr_substep(const GpdParams& P, const GpdCtbr& B, const PL& Q, const GpdStepCfg& C, const uint32_t flags,
                                             const bool drag, const float cmd[4], Carry& c, float& avx, float& avy, float& avz) {
    Kin& k = c.k;
    float rpm[4], g[4];
    gpd_ctbr_rate_loop(&B, P.M, P.J[0], P.J[1], P.J[2], cmd, k.wx, k.wy, k.wz, rpm);
#pragma unroll
    for (int i = 0; i < 4; ++i) g[i] = thrust_dev(Q, rpm[i]);
    const float drag_sum = drag ? ((c.l0 + c.l1) + c.l2) + c.l3 : 0.0f;
    substep<EXT, AV>(Q, C.pyb_dt, flags, g, drag_sum, 0.0f, k, avx, avy, avz);
    c.l0 = rpm[0]; c.l1 = rpm[1]; c.l2 = rpm[2]; c.l3 = rpm[3];
}
// the S sub-steps of one control step: only the last one's world angular velocity is observed
template <bool EXT, class PL>
__device__ __forceinline__ void ctbr_substeps(const GpdParams& P, const GpdCtbr& B, const PL& Q, const GpdStepCfg& C, const uint32_t flags,
                                              const bool drag, const float cmd[4], Carry& c, float& avx, float& avy, float& avz) {
    for (int ss = 1; ss < C.substeps; ++ss) ctbr_substep<EXT, false>(P, B, Q, C, flags, drag, cmd, c, avx, avy, avz);
    ctbr_substep<EXT, true>(P, B, Q, C, flags, drag, cmd, c, avx, avy, avz);
}

template <int MODE, bool EXT, bool PLANT>
__global__ __launch_bounds__(kBlock) void gpd_rollout_ctbr_kernel(
    const GpdParams P, const GpdCtbr B, float* __restrict__ kin, float* __restrict__ last_rpm, int32_t* __restrict__ step_counter,
    uint8_t* __restrict__ bad, const uint32_t ld32, const GpdStepCfg C, const float* __restrict__ rows, const int64_t rstride,
    const float* __restrict__ plant, float* __restrict__ obs12, const int64_t ostride, float* __restrict__ cmd_out, const int64_t cstride,
    const int K) {
    const uint32_t n = blockIdx.x * static_cast<uint32_t>(kBlock) + threadIdx.x;
    if (n >= static_cast<uint32_t>(C.num_envs)) return;
    const GpdState S{kin, last_rpm, nullptr, step_counter, static_cast<int64_t>(ld32), nullptr, nullptr, nullptr, 0, 0, bad};
    const uint32_t flags = EXT ? C.physics_flags : 0u;
    Lane L;
    L.n = n; L.env = n; L.tid = threadIdx.x; L.le = threadIdx.x; L.d = 0; L.base = threadIdx.x; L.active = true; L.shfl = false;
    Carry c;
    float tgx, tgy, tgz;
    load_carry<false, EXT, false>(S, C, flags, L, kin, nullptr, c, tgx, tgy, tgz, nullptr);     // (no task: a readable dummy target)
    plant_t<PLANT> Q = plant_of<PLANT>(P, plant, S.ld, n * 4u);
    Kin& k = c.k;
    const bool drag = EXT && (flags & GPD_PHYS_DRAG);
    float avx = 0.0f, avy = 0.0f, avz = 0.0f;
    CtbrRow row = ctbr_row<MODE>(rows, n);
    for (int t = 0; t < K; ++t) {
        // the NEXT step's row is requested before this step's arithmetic (a held row -- stride 0 -- is read again, a cache hit)
        const CtbrRow nx = ctbr_row<MODE>(rows + (t + 1 < K ? t + 1 : t) * rstride, n);
        float cmd[4];
        if constexpr (MODE == GPD_CTBR_POS)        // pos = a.xyz, vel = b.zw | c.x (rpy and its rates: ignored, as in the reference)
            gpd_ctbr_outer(&B, k.px, k.py, k.pz, k.qx, k.qy, k.qz, k.qw, k.vx, k.vy, k.vz, row.a.x, row.a.y, row.a.z, row.b.z, row.b.w, row.c.x, cmd);
        else { cmd[0] = row.a.x; cmd[1] = row.a.y; cmd[2] = row.a.z; cmd[3] = row.a.w; }
        if (cmd_out) *reinterpret_cast<float4*>(reinterpret_cast<char*>(cmd_out + t * cstride) + n * 16u) = make_float4(cmd[0], cmd[1], cmd[2], cmd[3]);
        // ---- S sub-steps, the rate loop in each: the command is held, the body rates are the integrator's own
        ctbr_substeps<EXT>(P, B, Q, C, flags, drag, cmd, c, avx, avy, avz);
        quat_to_rpy(k.qx, k.qy, k.qz, k.qw, c.roll, c.pitch, c.yaw);
        c.counter += C.substeps;
        if (ostride != 0 || t == K - 1) store_obs12(obs12 + t * ostride, n, k.px, k.py, k.pz, c.roll, c.pitch, c.yaw, k.vx, k.vy, k.vz, avx, avy, avz);
        row = nx;
    }
    store_carry<false>(S, L, c);
}

}  // namespace

extern "C" int gpd_sizeof_ctbr(int32_t* size_out) {
    if (!size_out) return Refuse{"gpd_sizeof_ctbr"}(GPD_EINVAL, "NULL size_out");
    *size_out = static_cast<int32_t>(sizeof(GpdCtbr));
    return 0;
}

extern "C" int gpd_ctbr(const GpdCtbr* ctbr, const float* cur_pos, const float* cur_quat, const float* cur_vel, const float* target_pos,
                        const float* target_vel, float* cmd, int32_t n, void* stream) {
    const Refuse bad{"gpd_ctbr"};
    if (!ctbr || !cur_pos || !cur_quat || !cur_vel || !target_pos || !cmd) return bad(GPD_EINVAL, "NULL argument");
    if (n <= 0) return bad(GPD_EINVAL, "n must be positive");
    if (n > (1 << 26)) return bad(GPD_ERANGE, "more than 2^26 drones per launch (32-bit byte offsets)");
    if (misaligned16(cur_quat) || misaligned16(cmd)) return bad(GPD_EINVAL, "cur_quat and cmd must be 16-byte aligned");
    hipLaunchKernelGGL(gpd_ctbr_kernel, dim3(blocks_for(n, kBlock)), dim3(kBlock), 0, static_cast<hipStream_t>(stream), *ctbr, cur_pos, cur_quat,
                       cur_vel, target_pos, target_vel, cmd, n);
    return launched(bad.who);
}

extern "C" int gpd_rollout_ctbr(const GpdParams* params, const GpdCtbr* ctbr, const GpdState* state, const GpdStepCfg* cfg, int32_t mode,
                                const float* rows, int64_t row_step_stride, const float* plant_rows, float* obs12, int64_t obs_step_stride,
                                float* cmd_out, int32_t num_steps, void* stream) {
    const Refuse bad{"gpd_rollout_ctbr"};
    if (!params || !ctbr || !state || !cfg) return bad(GPD_EINVAL, "NULL params/ctbr/state/cfg");
    if (int rc = check_state(bad, state)) return rc;
    if (!rows || !obs12) return bad(GPD_EINVAL, "NULL rows/obs12");
    if (mode != GPD_CTBR_CMD && mode != GPD_CTBR_POS) return bad(GPD_EINVAL, "unknown mode (GPD_CTBR_CMD or GPD_CTBR_POS)");
    if (int rc = check_steps(bad, num_steps, row_step_stride, obs_step_stride)) return rc;
    if (int rc = check_flags(bad, cfg)) return rc;
    // what the kernel serves, in front of the remaining shared checks (a configuration outside it answers GPD_ENOTSUP)
    if (cfg->drones_per_env != 1) return bad(GPD_ENOTSUP, "aviaries of one drone only");
    if (cfg->task != GPD_TASK_NONE || cfg->auto_reset) return bad(GPD_ENOTSUP, "GPD_TASK_NONE without auto-reset only");
    if (cfg->act_type != GPD_ACT_RAW_RPM && cfg->act_type != GPD_ACT_DIRECT_RPM)
        return bad(GPD_ENOTSUP, "act_type GPD_ACT_RAW_RPM or GPD_ACT_DIRECT_RPM (the rate loop's output is RPMs)");
    if ((cfg->physics_flags & GPD_PHYS_DW) || state->dw_force) return bad(GPD_ENOTSUP, "downwash needs mates");
    if (int rc = check_positive(bad, cfg)) return rc;
    const int64_t N = cfg->num_envs;
    if (int rc = check_extent(bad, N, state->ld)) return rc;
    if (int rc = check_needs(bad, params, state, cfg, nullptr, nullptr)) return rc;
    const int64_t width = mode == GPD_CTBR_POS ? 12 : 4;
    if ((row_step_stride != 0 && row_step_stride < width * N) || (obs_step_stride != 0 && obs_step_stride < 12 * N))
        return bad(GPD_EINVAL, "a non-zero step stride must cover a step's rows (4*num_envs commands or 12*num_envs targets; 12*num_envs for obs12)");
    if ((row_step_stride & 3) || (obs_step_stride & 3)) return bad(GPD_EINVAL, "step strides must be multiples of 4 floats (16-byte rows)");
    if (misaligned16(rows) || misaligned16(obs12) || misaligned16(plant_rows) || misaligned16(cmd_out))
        return bad(GPD_EINVAL, "rows, obs12, plant_rows and cmd_out must be 16-byte aligned");
    if (cmd_out && cmd_out == rows) return bad(GPD_EINVAL, "cmd_out must not alias rows");
    if (!(cfg->ctrl_dt > 0.0f) || !(cfg->pyb_dt > 0.0f)) return bad(GPD_EINVAL, "pyb_dt and ctrl_dt must be positive");
    GpdStepCfg C = *cfg;
    C.target_per_env = 0; C.init_per_env = 0; C.auto_reset = 0; C.task = GPD_TASK_NONE; C.drones_per_env = 1;
    const bool ext = (C.physics_flags & 31u) != 0;
    const int64_t cmd_stride = mode == GPD_CTBR_POS ? 4 * N : row_step_stride;
    const dim3 grid(blocks_for(N, kBlock));
    hipStream_t st = static_cast<hipStream_t>(stream);
    auto launch = [&](auto mode_) {
        with_ext_plant(ext, plant_rows != nullptr, [&](auto ext_, auto plant_) {
            hipLaunchKernelGGL((gpd_rollout_ctbr_kernel<decltype(mode_)::value, decltype(ext_)::value, decltype(plant_)::value>), grid, dim3(kBlock), 0, st,
                               *params, *ctbr, state->kin, state->last_rpm, state->step_counter, state->bad, static_cast<uint32_t>(state->ld), C, rows,
                               row_step_stride, plant_rows, obs12, obs_step_stride, cmd_out, cmd_stride, num_steps);
        });
    };
    if (mode == GPD_CTBR_POS) launch(Const<GPD_CTBR_POS>{}); else launch(Const<GPD_CTBR_CMD>{});
    return launched(bad.who);
}
