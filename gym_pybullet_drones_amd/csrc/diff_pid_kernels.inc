// diff_pid_kernels.inc -- the differentiable rollout through the DSLPID loop (pulled into abi.hip after diff_kernels.inc; DESIGN.md
// section 3.16):
//   gpd_rollout_tape_pid_kernel   gpd_rollout for the three DSLPID action types of single-drone aviaries -- the same load_carry /
//                                 map_action<true, ..> / env_step / store_carry code, so the same bits -- that also records, before every
//                                 env step, the 13 kinematic floats and the nine controller members the step starts from (22 floats =
//                                 88 B per drone-step).  The cached roll / pitch / yaw are NOT taped: at the top of every step they are
//                                 quat_to_rpy of the state's quaternion (the launch's first step computes them from the loaded state, the
//                                 tail of env_step from the state it leaves, no auto-reset here), and quat_to_rpy rounds identically in
//                                 every inlined copy (gpd_common.inc), so the sweep recomputes them from the taped quaternion bit for bit;
//   gpd_rollout_vjp_pid_kernel    the reverse sweep: one lane per drone, steps K-1 .. 0, the cotangents of the state (13) and of the
//                                 members (9) in registers.  Per step: the sub-steps' adjoint (substep_vjp<false, ..> of diff_kernels.inc
//                                 with its S(S+1)/2 recomputations), rotor thrust -> RPM, the controller (dslpid_vjp.inc), the target
//                                 mapping of the action type, and R(q) / rpy(q) of the step's start state into the quaternion's cotangent.
//                                 <.., GG>: the lane also sums the cotangents of the 18 gains over the sweep and stores them once after
//                                 the loop ([18][ld], per drone: the binding sums over drones).  No atomics: one writer per word.
// The tape, for any ld, keeps every 16-byte access aligned: three blocks of K planes of float4[ld] (P | Q | V, the planes of
// GpdState.kin) and then K blocks of ten rows of float[ld] (body rate z | the nine members).
#include "dslpid_vjp.inc"

namespace {

constexpr int kTapePidRows = 22;       // floats per drone-step

// drone n's step t of the tape: the three planes through planes_store / planes_load, the ten rows through the member-row helpers
__device__ __forceinline__ void tape_pid_store(float* __restrict__ tape, int64_t ld, int K, int t, uint32_t n, const Kin& k, const Pid& s) {
    float* rows = tape + (12 * static_cast<int64_t>(K) + 10 * static_cast<int64_t>(t)) * ld;
    planes_store(tape + (4 * static_cast<int64_t>(t)) * ld, tape + (4 * (static_cast<int64_t>(K) + t)) * ld,
                 tape + (4 * (2 * static_cast<int64_t>(K) + t)) * ld, rows, n, k);
    members_store(rows + ld, ld, n * 4u, s);
}
__device__ __forceinline__ void tape_pid_load(const float* __restrict__ tape, int64_t ld, int K, int t, uint32_t n, Kin& k, Pid& s) {
    const float* rows = tape + (12 * static_cast<int64_t>(K) + 10 * static_cast<int64_t>(t)) * ld;
    k = planes_load(tape + (4 * static_cast<int64_t>(t)) * ld, tape + (4 * (static_cast<int64_t>(K) + t)) * ld,
                    tape + (4 * (2 * static_cast<int64_t>(K) + t)) * ld, rows, n);
    members_load(rows + ld, ld, n * 4u, s);
}

// ------------------------------------------------------------------------------------------------
// the taped forward
// ------------------------------------------------------------------------------------------------
template <int AW>
__global__ __launch_bounds__(kBlock) void gpd_rollout_tape_pid_kernel(const GpdParams P, const GpdState S, const GpdStepCfg C, const int K, const int64_t a_stride,
                                                                      const int64_t o_stride, const int64_t e_stride,
                                                                      const float* __restrict__ actions, const float* __restrict__ target_pos,
                                                                      float* __restrict__ obs12, float* __restrict__ reward,
                                                                      uint8_t* __restrict__ terminated, uint8_t* __restrict__ truncated,
                                                                      float* __restrict__ tape) {
    const Lane L = tape_lane(static_cast<uint32_t>(C.num_envs));
    const int64_t ld = S.ld;
    Carry c;
    float tgx, tgy, tgz;
    load_carry<true, false, false>(S, C, 0u, L, target_pos, nullptr, c, tgx, tgy, tgz, nullptr);
    quat_to_rpy(c.k.qx, c.k.qy, c.k.qz, c.k.qw, c.roll, c.pitch, c.yaw);
    for (int t = 0; t < K; ++t, actions += a_stride, obs12 += o_stride, reward += e_stride, terminated += e_stride, truncated += e_stride) {
        const float4 act = load_action<AW>(actions, L.n);
        if (L.active) tape_pid_store(tape, ld, K, t, L.n, c.k, c.s);
        StepOut out;
        env_step<true, false, false, AW>(P, C, 0u, 1, L, act, tgx, tgy, tgz, false, nullptr, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f,
                                         nullptr, nullptr, c, out);
        tape_step_store(L, out, obs12, reward, terminated, truncated);
    }
    if (L.active) store_carry<true>(S, L, c);
}

// ------------------------------------------------------------------------------------------------
// the reverse sweep
// ------------------------------------------------------------------------------------------------
struct NoGains {};
template <bool GG> using gain_cot_t = std::conditional_t<GG, GpdDslGainCot, NoGains>;

template <int AW, bool GG>
__global__ __launch_bounds__(kBlock) void gpd_rollout_vjp_pid_kernel(const GpdParams P, const GpdStepCfg C, const int64_t ld, const int K,
                                                                     const float* __restrict__ actions, const int64_t a_stride,
                                                                     const float* __restrict__ target_pos, const float* __restrict__ tape,
                                                                     const float* __restrict__ g_obs12, const int64_t o_stride,
                                                                     const float* __restrict__ g_reward, const int64_t e_stride,
                                                                     float* __restrict__ g_kin, float* __restrict__ g_pid,
                                                                     float* __restrict__ g_actions, float* __restrict__ g_gains) {
    const uint32_t N = static_cast<uint32_t>(C.num_envs);
    const uint32_t n = blockIdx.x * kBlock + threadIdx.x;
    if (n >= N) return;
    const uint32_t off4 = n * 4u;
    const bool has_task = C.task != GPD_TASK_NONE;
    const float* tp = target_pos + (C.target_per_env ? static_cast<size_t>(n) * 3 : 0);      // (task NONE: a readable dummy)
    const float tgx = tp[0], tgy = tp[1], tgz = tp[2];
    const float h = C.pyb_dt;
    const int S = C.substeps;
    Kin A = kin_load(g_kin, ld, n);                            // cotangent of the state after the step in hand
    GpdDslOutCot o;                                            // ... and of the members after it (the RPMs' slots: per step)
    members_load(g_pid, ld, off4, o);
    gain_cot_t<GG> G{};                                        // GG: cotangents of the 18 gains, summed over the sweep
    NoCot no_plant;
    for (int t = K - 1; t >= 0; --t) {
        Carry c{};
        tape_pid_load(tape, ld, K, t, n, c.k, c.s);
        const Kin k0 = c.k;
        const Pid s0 = c.s;
        const float4 act = load_action<AW>(actions + t * a_stride, n);
        quat_to_rpy(k0.qx, k0.qy, k0.qz, k0.qw, c.roll, c.pitch, c.yaw);
        const float roll0 = c.roll, pitch0 = c.pitch, yaw0 = c.yaw;
        float rpm[4], g[4];
        map_action<true, AW, -1>(P, C, act, c, rpm, g);        // (the forward's controller call: its RPMs and thrust deviations)
        float go[12];
        if (g_obs12) {
            const f4u* row = reinterpret_cast<const f4u*>(g_obs12 + t * o_stride + static_cast<size_t>(n) * 12);
            const f4u r0 = row[0], r1 = row[1], r2 = row[2];
            go[0] = r0.x; go[1] = r0.y; go[2] = r0.z; go[3] = r0.w; go[4] = r1.x; go[5] = r1.y; go[6] = r1.z; go[7] = r1.w;
            go[8] = r2.x; go[9] = r2.y; go[10] = r2.z; go[11] = r2.w;
        } else {
#pragma unroll
            for (int i = 0; i < 12; ++i) go[i] = 0.0f;
        }
        const float grew = (g_reward && has_task) ? g_reward[t * e_stride + n] : 0.0f;
        // ---- the sub-steps, as gpd_rollout_vjp_kernel<false, ..> undoes them
        float ag[4] = {0.0f, 0.0f, 0.0f, 0.0f};
        float d0, d1, d2;
        for (int j = S - 1; j >= 0; --j) {
            Kin k = k0;                                        // the state sub-step j started from: j forward sub-steps from the tape
            for (int i = 0; i < j; ++i) substep<false, false>(P, h, 0u, g, 0.0f, 0.0f, k, d0, d1, d2);
            float a_drag = 0.0f;
            if (j == S - 1) {
                Kin kp = k;
                substep<false, false>(P, h, 0u, g, 0.0f, 0.0f, kp, d0, d1, d2);
                outputs_vjp(kp, go, grew, tgx, tgy, tgz, A);
                substep_vjp<false, true>(P, h, 0u, g, 0.0f, k, A, go[9], go[10], go[11], ag, a_drag, no_plant);
            } else {
                substep_vjp<false, false>(P, h, 0u, g, 0.0f, k, A, 0.0f, 0.0f, 0.0f, ag, a_drag, no_plant);
            }
        }
        // ---- thrust_dev: g_i = KF (rpm_i - h)(rpm_i + h) + resid
        o.rpm0 = ag[0] * (2.0f * P.KF * rpm[0]); o.rpm1 = ag[1] * (2.0f * P.KF * rpm[1]);
        o.rpm2 = ag[2] * (2.0f * P.KF * rpm[2]); o.rpm3 = ag[3] * (2.0f * P.KF * rpm[3]);
        // ---- the controller's inputs, map_action<true, ..>'s expressions
        const Mat3 R = quat_to_mat(k0.qx, k0.qy, k0.qz, k0.qw);
        GpdDslVars X;
        X.px = k0.px; X.py = k0.py; X.pz = k0.pz; X.vx = k0.vx; X.vy = k0.vy; X.vz = k0.vz;
        X.r00 = R.r00; X.r01 = R.r01; X.r02 = R.r02; X.r10 = R.r10; X.r11 = R.r11; X.r12 = R.r12; X.r20 = R.r20; X.r21 = R.r21; X.r22 = R.r22;
        X.roll = roll0; X.pitch = pitch0; X.yaw = yaw0;
        X.tx = k0.px; X.ty = k0.py; X.tz = k0.pz; X.tyaw = 0.0f; X.tvx = 0.0f; X.tvy = 0.0f; X.tvz = 0.0f;
        X.ipx = s0.ipx; X.ipy = s0.ipy; X.ipz = s0.ipz; X.lr = s0.lr; X.lp = s0.lp; X.ly = s0.ly; X.irx = s0.irx; X.iry = s0.iry; X.irz = s0.irz;
        // (what the target mappings' adjoints need of them)
        float dx = 0.0f, dy = 0.0f, dz = 0.0f, id = 0.0f, in = 0.0f, sp = 0.0f;
        bool inside = true, moving = false;
        if (AW == 3) {
            dx = act.x - k0.px; dy = act.y - k0.py; dz = act.z - k0.pz;
            const float dd = fmaf(dz, dz, fmaf(dy, dy, dx * dx));
            inside = fast_sqrt(dd) <= 1.0f;
            id = fast_rsq(dd);
            X.tx = inside ? act.x : fmaf(dx, id, k0.px); X.ty = inside ? act.y : fmaf(dy, id, k0.py); X.tz = inside ? act.z : fmaf(dz, id, k0.pz);
        } else if (AW == 4) {
            const float nn2 = fmaf(act.z, act.z, fmaf(act.y, act.y, act.x * act.x));
            sp = P.speed_limit * fabsf(act.w);
            moving = nn2 != 0.0f;
            in = fast_rsq(nn2);
            X.tvx = moving ? sp * (act.x * in) : 0.0f; X.tvy = moving ? sp * (act.y * in) : 0.0f; X.tvz = moving ? sp * (act.z * in) : 0.0f;
            X.tyaw = yaw0;
        } else {
            X.tz = fmaf(0.1f, act.x, k0.pz);
        }
        GpdDslVars a;
        if constexpr (GG) gpd_dslpid_vjp(&P, C.ctrl_dt, C.inv_ctrl_dt, &X, &o, &a, &G);
        else gpd_dslpid_vjp(&P, C.ctrl_dt, C.inv_ctrl_dt, &X, &o, &a, nullptr);
        // ---- the target mapping: the action's gradient, and what the targets pass on to the state
        float ga0 = 0.0f, ga1 = 0.0f, ga2 = 0.0f, ga3 = 0.0f;
        float tpx = a.tx, tpy = a.ty, tpz = a.tz;                  // cotangent the target position hands to the position
        float a_yaw = a.yaw;
        if (AW == 3) {
            // inside the 1 m limit the target is the action; outside it p + d / |d|: (I - dd^T) / |d| towards the action, I minus that to p
            const float ux = dx * id, uy = dy * id, uz = dz * id;
            const float pr = fmaf(uz, a.tz, fmaf(uy, a.ty, ux * a.tx));
            const float ox = id * fmaf(-ux, pr, a.tx), oy = id * fmaf(-uy, pr, a.ty), oz = id * fmaf(-uz, pr, a.tz);
            ga0 = inside ? a.tx : ox; ga1 = inside ? a.ty : oy; ga2 = inside ? a.tz : oz;
            tpx = inside ? 0.0f : a.tx - ox; tpy = inside ? 0.0f : a.ty - oy; tpz = inside ? 0.0f : a.tz - oz;
        } else if (AW == 4) {
            // tv = speed_limit |a_w| a_xyz / |a_xyz|: exactly zero where a_xyz = 0;  tyaw = the current yaw
            const float ux = act.x * in, uy = act.y * in, uz = act.z * in;
            const float pr = fmaf(uz, a.tvz, fmaf(uy, a.tvy, ux * a.tvx));
            const float sc = sp * in;
            const float sg = act.w > 0.0f ? P.speed_limit : (act.w < 0.0f ? -P.speed_limit : 0.0f);
            ga0 = moving ? sc * fmaf(-ux, pr, a.tvx) : 0.0f; ga1 = moving ? sc * fmaf(-uy, pr, a.tvy) : 0.0f;
            ga2 = moving ? sc * fmaf(-uz, pr, a.tvz) : 0.0f; ga3 = moving ? sg * pr : 0.0f;
            a_yaw += a.tyaw;
        } else {
            ga0 = 0.1f * a.tz;                                 // tz = 0.1 a + pz
        }
        // ---- into the state's cotangent: directly, through R(q) and through rpy(q)
        A.px += a.px + tpx; A.py += a.py + tpy; A.pz += a.pz + tpz;
        A.vx += a.vx; A.vy += a.vy; A.vz += a.vz;
        mat_vjp(k0.qx, k0.qy, k0.qz, k0.qw, a.r00, a.r01, a.r02, a.r10, a.r11, a.r12, a.r20, a.r21, a.r22, A.qx, A.qy, A.qz, A.qw);
        float rqx, rqy, rqz, rqw;
        rpy_vjp(k0.qx, k0.qy, k0.qz, k0.qw, a.roll, a.pitch, a_yaw, rqx, rqy, rqz, rqw);
        A.qx += rqx; A.qy += rqy; A.qz += rqz; A.qw += rqw;
        o.ipx = a.ipx; o.ipy = a.ipy; o.ipz = a.ipz; o.lr = a.lr; o.lp = a.lp; o.ly = a.ly; o.irx = a.irx; o.iry = a.iry; o.irz = a.irz;
        float* dst = g_actions + (static_cast<size_t>(t) * N + n) * AW;
        if (AW == 4) *reinterpret_cast<f4v*>(dst) = f4v{ga0, ga1, ga2, ga3};
        else if (AW == 3) { dst[0] = ga0; dst[1] = ga1; dst[2] = ga2; }
        else dst[0] = ga0;
    }
    kin_store(g_kin, ld, n, A);
    members_store(g_pid, ld, off4, o);
    if constexpr (GG) {
        st_row(g_gains, ld, 0, off4, G.pf0); st_row(g_gains, ld, 1, off4, G.pf1); st_row(g_gains, ld, 2, off4, G.pf2);
        st_row(g_gains, ld, 3, off4, G.if0); st_row(g_gains, ld, 4, off4, G.if1); st_row(g_gains, ld, 5, off4, G.if2);
        st_row(g_gains, ld, 6, off4, G.df0); st_row(g_gains, ld, 7, off4, G.df1); st_row(g_gains, ld, 8, off4, G.df2);
        st_row(g_gains, ld, 9, off4, G.pt0); st_row(g_gains, ld, 10, off4, G.pt1); st_row(g_gains, ld, 11, off4, G.pt2);
        st_row(g_gains, ld, 12, off4, G.it0); st_row(g_gains, ld, 13, off4, G.it1); st_row(g_gains, ld, 14, off4, G.it2);
        st_row(g_gains, ld, 15, off4, G.dt0); st_row(g_gains, ld, 16, off4, G.dt1); st_row(g_gains, ld, 17, off4, G.dt2);
    } else {
        (void)g_gains;
    }
}

// act_type -> the action row's width: both kernels of this file are launched as launch(aw)
template <class F>
void diff_pid_dispatch(const GpdStepCfg& c, F&& launch) {
    if (c.act_type == GPD_ACT_PID) launch(Const<3>{});
    else if (c.act_type == GPD_ACT_VEL) launch(Const<4>{});
    else launch(Const<1>{});
}

}  // namespace

extern "C" {

int gpd_rollout_tape_pid_floats(const GpdStepCfg* cfg, int32_t num_steps, int64_t ld, int64_t* floats_out) {
    // 13 kinematic floats + 9 members per env step
    return tape_floats_impl(Refuse{"gpd_rollout_tape_pid_floats"}, DiffFamily::PID, cfg, num_steps, ld, kTapePidRows, 0, floats_out);
}

int gpd_rollout_tape_pid(const GpdParams* params, const GpdState* state, const GpdStepCfg* cfg, int32_t num_steps, const float* actions,
                         int64_t action_step_stride, const float* target_pos, float* obs12, int64_t obs_step_stride, float* reward,
                         uint8_t* terminated, uint8_t* truncated, int64_t env_step_stride, float* tape, void* stream) {
    const Refuse bad{"gpd_rollout_tape_pid"};
    GpdStepCfg c;
    GpdState s;
    if (int rc = tape_prologue(bad, DiffFamily::PID, params, state, cfg, num_steps, actions, action_step_stride, target_pos, obs12,
                               obs_step_stride, reward, terminated, truncated, env_step_stride, tape, c, s))
        return rc;
    const dim3 grid(blocks_for(c.num_envs, kBlock));
    diff_pid_dispatch(c, [&](auto aw) {
        hipLaunchKernelGGL((gpd_rollout_tape_pid_kernel<decltype(aw)::value>), grid, dim3(kBlock), 0, static_cast<hipStream_t>(stream), *params, s, c,
                           num_steps, action_step_stride, obs_step_stride, env_step_stride, actions, target_pos, obs12, reward, terminated,
                           truncated, tape);
    });
    return launched(bad.who);
}

int gpd_rollout_vjp_pid(const GpdParams* params, const GpdStepCfg* cfg, int64_t ld, int32_t num_steps, const float* actions,
                        int64_t action_step_stride, const float* target_pos, const float* tape, const float* g_obs12,
                        int64_t obs_step_stride, const float* g_reward, int64_t env_step_stride, float* g_kin, float* g_pid,
                        float* g_actions, float* g_gains, void* stream) {
    const Refuse bad{"gpd_rollout_vjp_pid"};
    if (!params || !cfg) return bad(GPD_EINVAL, "NULL params/cfg");
    if (!actions || !tape || !g_kin || !g_pid || !g_actions) return bad(GPD_EINVAL, "NULL actions/tape/g_kin/g_pid/g_actions");
    if (int rc = sweep_prologue(bad, DiffFamily::PID, params, cfg, ld, num_steps, action_step_stride, obs_step_stride, env_step_stride,
                                target_pos, tape, g_kin))
        return rc;
    if (misaligned16(g_pid) || misaligned16(g_gains)) return bad(GPD_EINVAL, "g_pid and g_gains must be 16-byte aligned");
    if (cfg->act_type == GPD_ACT_VEL && misaligned16(g_actions)) return bad(GPD_EINVAL, "g_actions must be 16-byte aligned (GPD_ACT_VEL rows are stored as float4)");
    GpdStepCfg c = *cfg;
    dummy_target(c, target_pos, tape);
    const dim3 grid(blocks_for(c.num_envs, kBlock));
    diff_pid_dispatch(c, [&](auto aw) {
        auto launch = [&](auto gg) {
            hipLaunchKernelGGL((gpd_rollout_vjp_pid_kernel<decltype(aw)::value, decltype(gg)::value>), grid, dim3(kBlock), 0,
                               static_cast<hipStream_t>(stream), *params, c, ld, num_steps, actions, action_step_stride, target_pos, tape,
                               g_obs12, obs_step_stride, g_reward, env_step_stride, g_kin, g_pid, g_actions, g_gains);
        };
        if (g_gains) launch(Const<true>{}); else launch(Const<false>{});
    });
    return launched(bad.who);
}

}  // extern "C"
