// mppi_ctbr.inc -- gpd_mppi_ctbr (include/gpd.h): gpd_mppi over thrust and body-rate commands.  The samples are CTBR commands (thrust
// [m/s^2] | body rates [rad/s]) and the model closes the body-rate loop inside every physics sub-step, as gpd_rollout_ctbr flies a
// command in GPD_CTBR_CMD without physics flags or a plant table.  Pulled into abi.hip behind mppi.inc and ctbr.inc: the noise, the
// cost's combination and the weight are mppi_math.inc, the rate loop is ctbr_math.inc, the sub-step gpd_common.inc.  DESIGN.md 3.19.
//
// The kernel has the shape of gpd_mppi_kernel (mppi.inc: one wave per drone, lane = sample, pass 1 / butterflies / pass 2, no atomics,
// no LDS, one writer per word) and carries GpdCtbr, 32 more wave-uniform words.  gpd_mppi_kernel itself is left as it is: as one
// template over the env step its four instantiations came out with another register allocation and schedule (DESIGN.md 3.19), so the
// two passes are stated here as device helpers -- the running cost of a state, the update from the stored costs -- around mppi.inc's
// mppi_action and butterflies.

namespace {

// the running cost of the state `k` after step h against the goal row g4; `ob`, `opitch`, `n_obst`: the drone's list (OBST)
template <bool OBST>
__device__ __forceinline__ float mppi_state_cost(const GpdMppi& Q, const Kin& k, const float4 g4, const bool last, const float* __restrict__ ob,
                                                 const int64_t opitch, const int n_obst) {
    const float ex = k.px - g4.x, ey = k.py - g4.y, ez = k.pz - g4.z;
    const float dp2 = fmaf(ez, ez, fmaf(ey, ey, ex * ex));
    const float v2 = fmaf(k.vz, k.vz, fmaf(k.vy, k.vy, k.vx * k.vx));
    const float w2 = fmaf(k.wz, k.wz, fmaf(k.wy, k.wy, k.wx * k.wx));
    const Mat3 R = quat_to_mat(k.qx, k.qy, k.qz, k.qw);
    float clear = GPD_OBST_INF;
    if constexpr (OBST) {
        for (int r = 0; r < n_obst; ++r) {
            const float* rec = ob + static_cast<int64_t>(r) * GPD_OBST_FLOATS * opitch;
            const float kw = rec[3 * opitch];
            const int kind = __builtin_amdgcn_readfirstlane(kw == kw ? static_cast<int>(kw) : GPD_OBST_NONE);
            float nx, ny, nz;
            const float d = gpd_obst_sdf(kind, rec[4 * opitch], rec[5 * opitch], rec[6 * opitch], k.px - rec[0], k.py - rec[opitch],
                                         k.pz - rec[2 * opitch], &nx, &ny, &nz);
            clear = d < clear ? d : clear;            // (false for a NaN from a record that is not finite)
        }
    }
    const float wp = last ? Q.w_pos * Q.w_term : Q.w_pos;
    return gpd_mppi_step_cost(wp, Q.w_vel, Q.w_tilt, Q.w_rate, OBST ? Q.w_obs : 0.0f, Q.obst_margin, Q.collision_radius, dp2, v2, R.m22, w2, clear);
}

// Between the passes and pass 2 for drone n: every lane reads back the costs it stored itself in cn[M]; minimum, weight sum,
// squared-weight sum and weighted cost sum as fixed-order butterflies; per step the regenerated noise, four butterflies, and lane 0
// stores u_out[h][n] (on + h * u_stride) as 16 bytes; at the end stats4[n].
__device__ __forceinline__ void mppi_update(const GpdMppi& Q, const int n, const uint32_t lane, const float* cn, const float* __restrict__ un,
                                            const int64_t u_stride, float* __restrict__ on, float4* __restrict__ stats4) {
    const int H = Q.horizon, batches = Q.samples >> 6;
    float smin = GPD_OBST_INF;
    for (int b = 0; b < batches; ++b) {
        const float S = cn[static_cast<uint32_t>(b) * 64u + lane];
        smin = (gpd_mppi_finite(S) && S < smin) ? S : smin;
    }
    smin = wave_min(smin);
    const float inv_lambda = 1.0f / Q.lambda;
    float sw = 0.0f, sww = 0.0f, sws = 0.0f, cnt = 0.0f;
    for (int b = 0; b < batches; ++b) {
        const float S = cn[static_cast<uint32_t>(b) * 64u + lane];
        const bool fin = gpd_mppi_finite(S);
        const float w = gpd_mppi_weight(S, smin, inv_lambda);
        sw += w;
        sww = fmaf(w, w, sww);
        sws += fin ? w * (S * kMppiSumScale) : 0.0f;            // (as gpd_mppi_kernel: no overflow of the sum)
        cnt += fin ? 1.0f : 0.0f;
    }
    sw = wave_sum(sw); sww = wave_sum(sww); sws = wave_sum(sws); cnt = wave_sum(cnt);
    const bool any = cnt > 0.0f;               // (then sw >= 1: the minimum's own weight)
    const float inv_sw = any ? 1.0f / sw : 0.0f;
    for (int h = 0; h < H; ++h) {
        const float4 u = *reinterpret_cast<const float4*>(un + h * u_stride);
        float ax = 0.0f, ay = 0.0f, az = 0.0f, aw = 0.0f;
        for (int b = 0; b < batches; ++b) {
            const uint32_t m = static_cast<uint32_t>(b) * 64u + lane;
            const float w = gpd_mppi_weight(cn[m], smin, inv_lambda);
            const float4 a = mppi_action(Q, static_cast<uint32_t>(n), m, static_cast<uint32_t>(h), u);
            ax = fmaf(w, a.x - u.x, ax); ay = fmaf(w, a.y - u.y, ay); az = fmaf(w, a.z - u.z, az); aw = fmaf(w, a.w - u.w, aw);
        }
        ax = wave_sum(ax); ay = wave_sum(ay); az = wave_sum(az); aw = wave_sum(aw);
        // (clamped once more, as gpd_mppi_kernel: with no finite sample the sums are 0 and this is clamp(u_in))
        const f4v out = {clampf(fmaf(ax, inv_sw, u.x), Q.act_lo[0], Q.act_hi[0]), clampf(fmaf(ay, inv_sw, u.y), Q.act_lo[1], Q.act_hi[1]),
                         clampf(fmaf(az, inv_sw, u.z), Q.act_lo[2], Q.act_hi[2]), clampf(fmaf(aw, inv_sw, u.w), Q.act_lo[3], Q.act_hi[3])};
        if (lane == 0) *reinterpret_cast<f4v*>(on + h * u_stride) = out;
    }
    if (lane == 0) stats4[n] = make_float4(smin, any ? mppi_mean_cost(sws, inv_sw) : GPD_OBST_INF, any ? (sw * sw) / sww : 0.0f, cnt);
}

// OBST: a list is given
template <bool OBST>
__global__ __launch_bounds__(kBlock) void gpd_mppi_ctbr_kernel(const GpdParams P, const GpdCtbr B, const GpdStepCfg C, const GpdMppi Q,
                                                               const float* __restrict__ kin, const int64_t ld, const int N,
                                                               const float* __restrict__ u_in, const int64_t u_stride,
                                                               const float* __restrict__ goal, const int64_t goal_stride,
                                                               const float* __restrict__ obst, const int n_obst, const int64_t obst_ld,
                                                               float* __restrict__ u_out, float* __restrict__ costs, float4* __restrict__ stats4) {
    const int wave = __builtin_amdgcn_readfirstlane(static_cast<int>(threadIdx.x) >> 6);
    const int n = static_cast<int>(blockIdx.x) * kMppiDrones + wave;          // this wave's drone: uniform
    if (n >= N) return;
    const uint32_t lane = threadIdx.x & 63u;
    const int H = Q.horizon, batches = Q.samples >> 6;
    // what the samples share, uniform: the start state (state.last_rpm is not read: the model has no drag), the nominal, the goal, the list
    const float4 kp = kin_P(kin, ld)[n], kq = kin_Q(kin, ld)[n], kv = kin_V(kin, ld)[n];
    const float kwz = kin[12 * ld + n];
    const float* const un = u_in + static_cast<int64_t>(n) * 4;
    const float* const gn = goal + static_cast<int64_t>(n) * 4;
    const int64_t opitch = obst_ld == 0 ? 1 : obst_ld;
    const float* const ob = OBST ? obst + (obst_ld == 0 ? 0 : n) : nullptr;
    float* const cn = costs + static_cast<int64_t>(n) * Q.samples;

    // ---- pass 1: the samples' costs ----
    for (int b = 0; b < batches; ++b) {
        const uint32_t m = static_cast<uint32_t>(b) * 64u + lane;
        Kin k{kp.x, kp.y, kp.z, kq.x, kq.y, kq.z, kq.w, kv.x, kv.y, kv.z, kp.w, kv.w, kwz};
        float S = 0.0f;
        for (int h = 0; h < H; ++h) {
            const float4 u = *reinterpret_cast<const float4*>(un + h * u_stride);
            const float4 g4 = *reinterpret_cast<const float4*>(gn + h * goal_stride);
            const float4 a = mppi_action(Q, static_cast<uint32_t>(n), m, static_cast<uint32_t>(h), u);
            // one control step on the held command, as gpd_rollout_ctbr_kernel's `sub` without drag: per sub-step the rate loop on the
            // integrator's own body rates (the controller's M and J are the airframe's), the rotor thrusts, the sub-step
            const float cmd[4] = {a.x, a.y, a.z, a.w};
            float d0, d1, d2;
            for (int ss = 0; ss < C.substeps; ++ss) {
                float rpm[4], g[4];
                gpd_ctbr_rate_loop(&B, P.M, P.J[0], P.J[1], P.J[2], cmd, k.wx, k.wy, k.wz, rpm);
#pragma unroll
                for (int i = 0; i < 4; ++i) g[i] = thrust_dev(P, rpm[i]);
                substep<false, false>(P, C.pyb_dt, 0u, g, 0.0f, 0.0f, k, d0, d1, d2);
            }
            S += mppi_state_cost<OBST>(Q, k, g4, h == H - 1, ob, opitch, n_obst);
        }
        cn[m] = S;
    }
    mppi_update(Q, n, lane, cn, un, u_stride, u_out + static_cast<int64_t>(n) * 4, stats4);
}

}  // namespace

extern "C" int gpd_mppi_ctbr(const GpdParams* params, const GpdCtbr* ctbr, const GpdState* state, const GpdStepCfg* cfg, const GpdMppi* mppi,
                             const float* u_in, int64_t u_step_stride, const float* goal, int64_t goal_step_stride, const float* obst,
                             int32_t n_obst, int64_t obst_ld, float* u_out, float* costs, float* stats4, void* stream) {
    const Refuse bad{"gpd_mppi_ctbr"};
    if (!params || !ctbr || !state || !cfg || !mppi) return bad(GPD_EINVAL, "NULL params/ctbr/state/cfg/mppi");
    if (!u_in || !goal || !u_out || !costs || !stats4) return bad(GPD_EINVAL, "NULL u_in/goal/u_out/costs/stats4");
    if (int rc = check_state(bad, state)) return rc;
    if (int rc = check_ranges(bad, cfg)) return rc;
    if (int rc = check_positive(bad, cfg)) return rc;
    if (int rc = check_flags(bad, cfg)) return rc;
    const int64_t N = static_cast<int64_t>(cfg->num_envs) * cfg->drones_per_env;
    if (int rc = check_extent(bad, N, state->ld)) return rc;
    // what the planning model is: gpd_mppi's, on the action types gpd_rollout_ctbr flies (the rate loop's output is RPMs)
    if (cfg->drones_per_env != 1) return bad(GPD_ENOTSUP, "aviaries of more than one drone are not planned for (drones_per_env must be 1)");
    if (cfg->physics_flags != 0u) return bad(GPD_ENOTSUP, "the planning model has no physics_flags (drag, ground effect, downwash, ground plane, damping)");
    if (cfg->task != GPD_TASK_NONE || cfg->auto_reset) return bad(GPD_ENOTSUP, "the planning model has no episode ends (task must be GPD_TASK_NONE, auto_reset 0)");
    if (cfg->act_type != GPD_ACT_RAW_RPM && cfg->act_type != GPD_ACT_DIRECT_RPM)
        return bad(GPD_ENOTSUP, "act_type GPD_ACT_RAW_RPM or GPD_ACT_DIRECT_RPM (the rate loop's output is RPMs)");
    const GpdMppi& q = *mppi;
    if (int rc = check_mppi_plan(bad, q, N, u_in, u_step_stride, goal, goal_step_stride, obst, n_obst, obst_ld, u_out, stats4)) return rc;
    auto launch = [&](auto ob) {
        hipLaunchKernelGGL((gpd_mppi_ctbr_kernel<decltype(ob)::value>), dim3(blocks_for(N, kMppiDrones)), dim3(kBlock), 0, static_cast<hipStream_t>(stream),
                           *params, *ctbr, *cfg, q, state->kin, state->ld, static_cast<int>(N), u_in, u_step_stride, goal, goal_step_stride, obst, n_obst,
                           obst_ld, u_out, costs, reinterpret_cast<float4*>(stats4));
    };
    if (obst != nullptr && n_obst > 0) launch(Const<true>{}); else launch(Const<false>{});
    return launched(bad.who);
}
