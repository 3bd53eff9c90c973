// mppi.inc -- gpd_mppi (include/gpd.h): sampling-based model-predictive control, M perturbed action sequences per drone rolled H env
// steps through the in-register physics, scored, and averaged with their softmax weights.  Pulled into abi.hip; the noise, the cost's
// combination and the weight are mppi_math.inc, the text a host program compiles too.  DESIGN.md section 3.15.
//
// One kernel, one launch, no atomics, one writer per word.  One 64-lane wave per drone, lane = sample, M / 64 samples per lane in
// sequence; a workgroup holds kBlock / 64 = 4 drones and a wave beyond N does nothing.  What a drone's samples share -- the start state,
// the nominal action of a step, the goal, the obstacle records (a per-aviary list too: the aviary IS the wave's drone) -- is read at
// wave-uniform addresses; a record's kind goes through v_readfirstlane, so a wave evaluates ONE shape per record.
//   pass 1   every lane rolls its samples and stores each one's total cost to costs[n][m] (256 contiguous bytes per wave and batch)
//   between  the lanes read their own costs back (never a runtime-indexed register array: that is scratch memory); minimum, weight
//            sum, squared-weight sum and weighted cost sum are xor-butterflies in a fixed order -- the same bits in every lane, call
//            after call
//   pass 2   per step the lanes REGENERATE their samples' noise (counter-based: nothing was stored), accumulate w (a - u) for the four
//            components, four butterflies, and lane 0 stores u_out[h][n] as 16 bytes; at the end stats4[n]
#include "obstacle_math.inc"
#include "mppi_math.inc"

namespace {

constexpr int kMppiDrones = kBlock / 64;          // drones (waves) per workgroup

// sum / minimum over the wave's 64 lanes, xor-butterfly 32, 16 .. 1: every lane ends with the same bits
__device__ __forceinline__ float wave_sum(float v) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off, 64);
    return v;
}
__device__ __forceinline__ float wave_min(float v) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v = fminf(v, __shfl_xor(v, off, 64));
    return v;
}

// the weighted cost sum is kept as sum w (S 2^-11): M <= 1024 finite costs of up to FLT_MAX (w_obs as a hard wall) then sum without an
// overflow, and a power of two changes no other bit
constexpr float kMppiSumScale = 4.8828125e-4f, kMppiSumUnscale = 2048.0f;
__device__ __forceinline__ float mppi_mean_cost(float sws, float inv_sw) { return fminf(sws * inv_sw * kMppiSumUnscale, 3.4028234e38f); }

// the action of sample m of drone n at step h: the clamped perturbation of the nominal u
__device__ __forceinline__ float4 mppi_action(const GpdMppi& Q, uint32_t n, uint32_t m, uint32_t h, const float4 u) {
    float z0, z1, z2, z3;
    gpd_mppi_normals(n, m, h, Q.iteration, Q.seed[0], Q.seed[1], &z0, &z1, &z2, &z3);
    return make_float4(gpd_mppi_perturb(u.x, Q.sigma[0], z0, Q.act_lo[0], Q.act_hi[0]), gpd_mppi_perturb(u.y, Q.sigma[1], z1, Q.act_lo[1], Q.act_hi[1]),
                       gpd_mppi_perturb(u.z, Q.sigma[2], z2, Q.act_lo[2], Q.act_hi[2]), gpd_mppi_perturb(u.w, Q.sigma[3], z3, Q.act_lo[3], Q.act_hi[3]));
}

// ACT: GPD_ACT_RPM or GPD_ACT_VEL (the latter runs DSLPID on lane-local copies of the drone's controller members); OBST: a list is given
template <int ACT, bool OBST>
__global__ __launch_bounds__(kBlock) void gpd_mppi_kernel(const GpdParams P, const GpdStepCfg C, const GpdMppi Q, const float* __restrict__ kin,
                                                          const float* __restrict__ pid, const int64_t ld, const int N,
                                                          const float* __restrict__ u_in, const int64_t u_stride,
                                                          const float* __restrict__ goal, const int64_t goal_stride,
                                                          const float* __restrict__ obst, const int n_obst, const int64_t obst_ld,
                                                          float* __restrict__ u_out, float* __restrict__ costs, float4* __restrict__ stats4) {
    constexpr bool PID = ACT == GPD_ACT_VEL;
    const int wave = __builtin_amdgcn_readfirstlane(static_cast<int>(threadIdx.x) >> 6);
    const int n = static_cast<int>(blockIdx.x) * kMppiDrones + wave;          // this wave's drone: uniform
    if (n >= N) return;
    const uint32_t lane = threadIdx.x & 63u;
    const int H = Q.horizon, batches = Q.samples >> 6;

    // ---- what the samples share: the start state (and the controller members), uniform ----
    const float4 kp = kin_P(kin, ld)[n], kq = kin_Q(kin, ld)[n], kv = kin_V(kin, ld)[n];
    const float kwz = kin[12 * ld + n];
    Pid s0{0, 0, 0, 0, 0, 0, 0, 0, 0};
    float roll0 = 0.0f, pitch0 = 0.0f, yaw0 = 0.0f;
    if constexpr (PID) {
        s0.ipx = pid[0 * ld + n]; s0.ipy = pid[1 * ld + n]; s0.ipz = pid[2 * ld + n];
        s0.lr = pid[3 * ld + n]; s0.lp = pid[4 * ld + n]; s0.ly = pid[5 * ld + n];
        s0.irx = pid[6 * ld + n]; s0.iry = pid[7 * ld + n]; s0.irz = pid[8 * ld + n];
        quat_to_rpy(kq.x, kq.y, kq.z, kq.w, roll0, pitch0, yaw0);           // (the rpy of the cached pose, as the rollout kernels' first step)
    }
    const float* const un = u_in + static_cast<int64_t>(n) * 4;
    const float* const gn = goal + static_cast<int64_t>(n) * 4;
    // the drone's list: float f of record r at ob[(r * 8 + f) * opitch] (a shared list is the pitch-1 case at aviary 0)
    const int64_t opitch = obst_ld == 0 ? 1 : obst_ld;
    const float* const ob = OBST ? obst + (obst_ld == 0 ? 0 : n) : nullptr;
    float* const cn = costs + static_cast<int64_t>(n) * Q.samples;

    // ---- pass 1: the samples' costs ----
    for (int b = 0; b < batches; ++b) {
        const uint32_t m = static_cast<uint32_t>(b) * 64u + lane;
        Carry c;
        c.k = Kin{kp.x, kp.y, kp.z, kq.x, kq.y, kq.z, kq.w, kv.x, kv.y, kv.z, kp.w, kv.w, kwz};
        c.s = s0;
        c.l0 = c.l1 = c.l2 = c.l3 = 0.0f; c.counter = 0; c.dw_in = 0.0f;
        c.roll = roll0; c.pitch = pitch0; c.yaw = yaw0;
        Kin& k = c.k;
        float S = 0.0f;
        for (int h = 0; h < H; ++h) {
            const float4 u = *reinterpret_cast<const float4*>(un + h * u_stride);
            const float4 g4 = *reinterpret_cast<const float4*>(gn + h * goal_stride);
            const float4 a = mppi_action(Q, static_cast<uint32_t>(n), m, static_cast<uint32_t>(h), u);
            // one env step, as gpd_rollout takes it: action -> RPM (DSLPID for VEL), the sub-steps, the rpy refresh
            float rpm[4], g[4], d0, d1, d2;
            map_action<PID, 4, ACT>(P, C, a, c, rpm, g);
            for (int ss = 0; ss < C.substeps; ++ss) substep<false, false>(P, C.pyb_dt, 0u, g, 0.0f, 0.0f, k, d0, d1, d2);
            if constexpr (PID) quat_to_rpy(k.qx, k.qy, k.qz, k.qw, c.roll, c.pitch, c.yaw);
            // the running cost of the state after the step
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
            const float wp = h == H - 1 ? Q.w_pos * Q.w_term : Q.w_pos;
            S += gpd_mppi_step_cost(wp, Q.w_vel, Q.w_tilt, Q.w_rate, OBST ? Q.w_obs : 0.0f, Q.obst_margin, Q.collision_radius, dp2, v2, R.m22, w2, clear);
        }
        cn[m] = S;
    }

    // ---- between the passes: minimum, then the weights' sums (every lane reads what it wrote itself) ----
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
        sws += fin ? w * (S * kMppiSumScale) : 0.0f;
        cnt += fin ? 1.0f : 0.0f;
    }
    sw = wave_sum(sw); sww = wave_sum(sww); sws = wave_sum(sws); cnt = wave_sum(cnt);
    const bool any = cnt > 0.0f;               // (then sw >= 1: the minimum's own weight)
    const float inv_sw = any ? 1.0f / sw : 0.0f;

    // ---- pass 2: the weighted mean of the clamped perturbations, step by step ----
    float* const on = u_out + static_cast<int64_t>(n) * 4;
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
        // (clamped once more: a convex combination of clamped actions is inside the bounds, its rounded sum only nearly; with no finite
        // sample the sums are 0 and this is clamp(u_in))
        const f4v out = {clampf(fmaf(ax, inv_sw, u.x), Q.act_lo[0], Q.act_hi[0]), clampf(fmaf(ay, inv_sw, u.y), Q.act_lo[1], Q.act_hi[1]),
                         clampf(fmaf(az, inv_sw, u.z), Q.act_lo[2], Q.act_hi[2]), clampf(fmaf(aw, inv_sw, u.w), Q.act_lo[3], Q.act_hi[3])};
        if (lane == 0) *reinterpret_cast<f4v*>(on + h * u_stride) = out;
    }
    if (lane == 0) stats4[n] = make_float4(smin, any ? mppi_mean_cost(sws, inv_sw) : GPD_OBST_INF, any ? (sw * sw) / sww : 0.0f, cnt);
}

// what gpd_mppi and gpd_mppi_ctbr refuse of the plan itself: the sampler, the buffers, the strides, the list (N: the drones)
[[maybe_unused]] int check_mppi_plan(Refuse bad, const GpdMppi& q, int64_t N, const float* u_in, int64_t u_step_stride, const float* goal,
                                     int64_t goal_step_stride, const float* obst, int32_t n_obst, int64_t obst_ld, const float* u_out,
                                     const float* stats4) {
    if (q.horizon < 1) return bad(GPD_EINVAL, "horizon must be >= 1");
    if (q.samples < 64 || q.samples > 1024 || q.samples % 64 != 0) return bad(GPD_EINVAL, "samples must be a multiple of 64 in 64 .. 1024");
    if (!(q.lambda > 0.0f) || !(q.lambda < GPD_OBST_INF)) return bad(GPD_EINVAL, "lambda must be positive and finite");
    for (int i = 0; i < 4; ++i) {
        if (!(q.sigma[i] >= 0.0f) || !(q.sigma[i] < GPD_OBST_INF)) return bad(GPD_EINVAL, "sigma must be non-negative and finite");
        if (!(q.act_lo[i] <= q.act_hi[i])) return bad(GPD_EINVAL, "act_lo must not exceed act_hi");
    }
    if (u_out == u_in) return bad(GPD_EINVAL, "u_out must not alias u_in");
    if (misaligned16(u_in) || misaligned16(u_out) || misaligned16(goal) || misaligned16(stats4))
        return bad(GPD_EINVAL, "u_in, u_out, goal and stats4 must be 16-byte aligned");
    if (u_step_stride % 4 != 0 || goal_step_stride % 4 != 0 || goal_step_stride < 0 || (goal_step_stride != 0 && goal_step_stride < 4 * N) ||
        u_step_stride < (q.horizon > 1 ? 4 * N : 0))
        return bad(GPD_EINVAL, "step strides must be multiples of 4 floats: u_step_stride >= 4 * num_envs, goal_step_stride 0 or >= 4 * num_envs");
    if (n_obst < 0 || n_obst > GPD_OBST_MAX) return bad(GPD_EINVAL, "n_obst must be in 0..1024");
    if (obst != nullptr && n_obst > 0 && obst_ld != 0 && obst_ld < N) return bad(GPD_EINVAL, "obst_ld must be 0 (one shared list) or >= num_envs (one list per aviary)");
    return 0;
}

}  // namespace

extern "C" int gpd_mppi(const GpdParams* params, const GpdState* state, const GpdStepCfg* cfg, const GpdMppi* mppi, const float* u_in,
                        int64_t u_step_stride, const float* goal, int64_t goal_step_stride, const float* obst, int32_t n_obst, int64_t obst_ld,
                        float* u_out, float* costs, float* stats4, void* stream) {
    const Refuse bad{"gpd_mppi"};
    if (!params || !state || !cfg || !mppi) return bad(GPD_EINVAL, "NULL params/state/cfg/mppi");
    if (!u_in || !goal || !u_out || !costs || !stats4) return bad(GPD_EINVAL, "NULL u_in/goal/u_out/costs/stats4");
    if (int rc = check_state(bad, state)) return rc;
    if (int rc = check_ranges(bad, cfg)) return rc;
    if (int rc = check_positive(bad, cfg)) return rc;
    if (int rc = check_flags(bad, cfg)) return rc;
    const int64_t N = static_cast<int64_t>(cfg->num_envs) * cfg->drones_per_env;
    if (int rc = check_extent(bad, N, state->ld)) return rc;
    // what the planning model is: single drones under the flag-less explicit integrator, no episode ends, rotor-level or velocity commands
    if (cfg->drones_per_env != 1) return bad(GPD_ENOTSUP, "aviaries of more than one drone are not planned for (drones_per_env must be 1)");
    if (cfg->physics_flags != 0u) return bad(GPD_ENOTSUP, "the planning model has no physics_flags (drag, ground effect, downwash, ground plane, damping)");
    if (cfg->task != GPD_TASK_NONE || cfg->auto_reset) return bad(GPD_ENOTSUP, "the planning model has no episode ends (task must be GPD_TASK_NONE, auto_reset 0)");
    if (cfg->act_type != GPD_ACT_RPM && cfg->act_type != GPD_ACT_VEL) return bad(GPD_ENOTSUP, "act_type must be GPD_ACT_RPM or GPD_ACT_VEL");
    if (int rc = check_needs(bad, params, state, cfg, nullptr, nullptr)) return rc;
    const GpdMppi& q = *mppi;
    if (int rc = check_mppi_plan(bad, q, N, u_in, u_step_stride, goal, goal_step_stride, obst, n_obst, obst_ld, u_out, stats4)) return rc;
    const bool has_obst = obst != nullptr && n_obst > 0;
    auto launch = [&](auto act, auto ob) {
        hipLaunchKernelGGL((gpd_mppi_kernel<decltype(act)::value, decltype(ob)::value>), dim3(blocks_for(N, kMppiDrones)), dim3(kBlock), 0,
                           static_cast<hipStream_t>(stream), *params, *cfg, q, state->kin, state->pid, state->ld, static_cast<int>(N), u_in,
                           u_step_stride, goal, goal_step_stride, obst, n_obst, obst_ld, u_out, costs, reinterpret_cast<float4*>(stats4));
    };
    auto with_obst = [&](auto act) { if (has_obst) launch(act, Const<true>{}); else launch(act, Const<false>{}); };
    if (cfg->act_type == GPD_ACT_VEL) with_obst(Const<static_cast<int>(GPD_ACT_VEL)>{}); else with_obst(Const<static_cast<int>(GPD_ACT_RPM)>{});
    return launched(bad.who);
}
