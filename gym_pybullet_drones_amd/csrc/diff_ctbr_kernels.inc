// diff_ctbr_kernels.inc -- the differentiable rollout through the thrust-and-body-rate loop (pulled into abi.hip after diff_kernels.inc
// and ctbr.inc; DESIGN.md section 3.18):
//   gpd_rollout_tape_ctbr_kernel   gpd_rollout_ctbr_kernel<MODE, false, PLANT>'s loop -- the same load_carry / gpd_ctbr_outer /
//                                  gpd_ctbr_rate_loop / substep / store_carry calls, so the same bits -- that also records, before every
//                                  control step, the 13 kinematic floats the step starts from (K blocks in the plane layout of
//                                  GpdState.kin, 52 B per drone-step; no rpm-sum row: drag is not served);
//   gpd_rollout_vjp_ctbr_kernel    the reverse sweep: one lane per drone, steps K-1 .. 0, the state's cotangent in 13 registers.  The RPMs
//                                  change every sub-step, so the recomputation of sub-step j's start state runs the rate loop in front of
//                                  each of its j forward sub-steps (S(S+1)/2 rate loops + sub-steps per step, as gpd_rollout_vjp's
//                                  sub-steps alone); then substep_vjp, then the rate loop's adjoint on that sub-step's own cotangents
//                                  (ctbr_vjp.inc): into the body rates' cotangent, and summed over the S sub-steps into the held
//                                  command's.  GPD_CTBR_POS: gpd_ctbr_outer_vjp on the step's start state turns the command's cotangent
//                                  into the target row's gradient and adds to the cotangents of position, quaternion and velocity.
//                                  <.., GG>: the lane also sums the cotangents of the 12 gains over the sweep and stores them once
//                                  ([12][ld], per drone: the binding sums over drones).  No atomics: one writer per word.
#include "ctbr_vjp.inc"

namespace {

// ------------------------------------------------------------------------------------------------
// the taped forward
// ------------------------------------------------------------------------------------------------
template <int MODE, bool PLANT>
__global__ __launch_bounds__(kBlock) void gpd_rollout_tape_ctbr_kernel(
    const GpdParams P, const GpdCtbr B, float* __restrict__ kin, float* __restrict__ last_rpm, int32_t* __restrict__ step_counter,
    uint8_t* __restrict__ bad, const uint32_t ld32, const GpdStepCfg C, const float* __restrict__ rows, const int64_t rstride,
    const float* __restrict__ plant, float* __restrict__ obs12, const int64_t ostride, float* __restrict__ cmd_out, const int64_t cstride,
    const int K, float* __restrict__ tape) {
    const uint32_t n = blockIdx.x * static_cast<uint32_t>(kBlock) + threadIdx.x;
    if (n >= static_cast<uint32_t>(C.num_envs)) return;
    const GpdState S{kin, last_rpm, nullptr, step_counter, static_cast<int64_t>(ld32), nullptr, nullptr, nullptr, 0, 0, bad};
    Lane L;
    L.n = n; L.env = n; L.tid = threadIdx.x; L.le = threadIdx.x; L.d = 0; L.base = threadIdx.x; L.active = true; L.shfl = false;
    Carry c;
    float tgx, tgy, tgz;
    load_carry<false, false, false>(S, C, 0u, L, kin, nullptr, c, tgx, tgy, tgz, nullptr);     // (no task: a readable dummy target)
    plant_t<PLANT> Q = plant_of<PLANT>(P, plant, S.ld, n * 4u);
    Kin& k = c.k;
    float avx = 0.0f, avy = 0.0f, avz = 0.0f;
    CtbrRow row = ctbr_row<MODE>(rows, n);
    for (int t = 0; t < K; ++t, tape += 13 * S.ld) {
        const CtbrRow nx = ctbr_row<MODE>(rows + (t + 1 < K ? t + 1 : t) * rstride, n);
        kin_store(tape, S.ld, n, k);
        float cmd[4];
        if constexpr (MODE == GPD_CTBR_POS)
            gpd_ctbr_outer(&B, k.px, k.py, k.pz, k.qx, k.qy, k.qz, k.qw, k.vx, k.vy, k.vz, row.a.x, row.a.y, row.a.z, row.b.z, row.b.w, row.c.x, cmd);
        else { cmd[0] = row.a.x; cmd[1] = row.a.y; cmd[2] = row.a.z; cmd[3] = row.a.w; }
        if (cmd_out) *reinterpret_cast<float4*>(reinterpret_cast<char*>(cmd_out + t * cstride) + n * 16u) = make_float4(cmd[0], cmd[1], cmd[2], cmd[3]);
        auto sub = [&](auto av) {
            float rpm[4], g[4];
            gpd_ctbr_rate_loop(&B, P.M, P.J[0], P.J[1], P.J[2], cmd, k.wx, k.wy, k.wz, rpm);
#pragma unroll
            for (int i = 0; i < 4; ++i) g[i] = thrust_dev(Q, rpm[i]);
            substep<false, decltype(av)::value>(Q, C.pyb_dt, 0u, g, 0.0f, 0.0f, k, avx, avy, avz);
            c.l0 = rpm[0]; c.l1 = rpm[1]; c.l2 = rpm[2]; c.l3 = rpm[3];
        };
        for (int ss = 1; ss < C.substeps; ++ss) sub(Const<false>{});
        sub(Const<true>{});
        quat_to_rpy(k.qx, k.qy, k.qz, k.qw, c.roll, c.pitch, c.yaw);
        c.counter += C.substeps;
        if (ostride != 0 || t == K - 1) store_obs12(obs12 + t * ostride, n, k.px, k.py, k.pz, c.roll, c.pitch, c.yaw, k.vx, k.vy, k.vz, avx, avy, avz);
        row = nx;
    }
    store_carry<false>(S, L, c);
}

// ------------------------------------------------------------------------------------------------
// the reverse sweep
// ------------------------------------------------------------------------------------------------
template <int MODE, bool PLANT, bool GG>
__global__ __launch_bounds__(kBlock) void gpd_rollout_vjp_ctbr_kernel(const GpdParams P, const GpdCtbr B, const GpdStepCfg C, const int64_t ld,
                                                                      const int K, const float* __restrict__ rows, const int64_t rstride,
                                                                      const float* __restrict__ plant, const float* __restrict__ tape,
                                                                      const float* __restrict__ g_obs12, const int64_t o_stride,
                                                                      float* __restrict__ g_kin, float* __restrict__ g_rows,
                                                                      float* __restrict__ g_gains) {
    const uint32_t N = static_cast<uint32_t>(C.num_envs);
    const uint32_t n = blockIdx.x * kBlock + threadIdx.x;
    if (n >= N) return;
    plant_t<PLANT> Q = plant_of<PLANT>(P, plant, ld, n * 4u);
    const float kf_plant = Q.KF;                               // the physics' KF; B.inv_kf is the controller's nominal one
    const float h = C.pyb_dt;
    const int S = C.substeps;
    Kin A = kin_load(g_kin, ld, n);                            // cotangent of the state after the step in hand
    float gk[9] = {0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f};      // GG: cotangents of k_p | k_d | k_rates, summed over the sweep
    float gr[3] = {0.0f, 0.0f, 0.0f};                          // ... and of k_rate
    NoCot no_plant;
    for (int t = K - 1; t >= 0; --t) {
        const Kin k0 = kin_load(tape + static_cast<int64_t>(t) * 13 * ld, ld, n);
        const CtbrRow row = ctbr_row<MODE>(rows + t * rstride, n);
        float cmd[4];
        if constexpr (MODE == GPD_CTBR_POS)
            gpd_ctbr_outer(&B, k0.px, k0.py, k0.pz, k0.qx, k0.qy, k0.qz, k0.qw, k0.vx, k0.vy, k0.vz, row.a.x, row.a.y, row.a.z, row.b.z, row.b.w, row.c.x, cmd);
        else { cmd[0] = row.a.x; cmd[1] = row.a.y; cmd[2] = row.a.z; cmd[3] = row.a.w; }
        float go[12];
        if (g_obs12 && (o_stride != 0 || t == K - 1)) {       // (stride 0: the forward kept the last step's rows only)
            const f4u* src = reinterpret_cast<const f4u*>(g_obs12 + t * o_stride + static_cast<size_t>(n) * 12);
            const f4u r0 = src[0], r1 = src[1], r2 = src[2];
            go[0] = r0.x; go[1] = r0.y; go[2] = r0.z; go[3] = r0.w; go[4] = r1.x; go[5] = r1.y; go[6] = r1.z; go[7] = r1.w;
            go[8] = r2.x; go[9] = r2.y; go[10] = r2.z; go[11] = r2.w;
        } else {
#pragma unroll
            for (int i = 0; i < 12; ++i) go[i] = 0.0f;
        }
        float acmd[4] = {0.0f, 0.0f, 0.0f, 0.0f};              // cotangent of the command the S sub-steps held
        float d0, d1, d2;
        for (int j = S - 1; j >= 0; --j) {
            Kin k = k0;                                        // the state sub-step j started from: j forward sub-steps from the tape
            float rpm[4], g[4];
            for (int i = 0; i < j; ++i) {
                gpd_ctbr_rate_loop(&B, P.M, P.J[0], P.J[1], P.J[2], cmd, k.wx, k.wy, k.wz, rpm);
#pragma unroll
                for (int r = 0; r < 4; ++r) g[r] = thrust_dev(Q, rpm[r]);
                substep<false, false>(Q, h, 0u, g, 0.0f, 0.0f, k, d0, d1, d2);
            }
            gpd_ctbr_rate_loop(&B, P.M, P.J[0], P.J[1], P.J[2], cmd, k.wx, k.wy, k.wz, rpm);
#pragma unroll
            for (int r = 0; r < 4; ++r) g[r] = thrust_dev(Q, rpm[r]);
            float ag[4] = {0.0f, 0.0f, 0.0f, 0.0f};
            float a_drag = 0.0f;
            if (j == S - 1) {
                // the step's outputs are functions of the state its LAST sub-step leaves (no reward here: its target is that position)
                Kin kp = k;
                substep<false, false>(Q, h, 0u, g, 0.0f, 0.0f, kp, d0, d1, d2);
                outputs_vjp(kp, go, 0.0f, kp.px, kp.py, kp.pz, A);
                substep_vjp<false, true>(Q, h, 0u, g, 0.0f, k, A, go[9], go[10], go[11], ag, a_drag, no_plant);
            } else {
                substep_vjp<false, false>(Q, h, 0u, g, 0.0f, k, A, 0.0f, 0.0f, 0.0f, ag, a_drag, no_plant);
            }
            float aw[3] = {0.0f, 0.0f, 0.0f};
            if constexpr (GG) gpd_ctbr_rate_loop_vjp(&B, P.M, P.J[0], P.J[1], P.J[2], kf_plant, cmd, k.wx, k.wy, k.wz, ag, acmd, aw, gr);
            else gpd_ctbr_rate_loop_vjp(&B, P.M, P.J[0], P.J[1], P.J[2], kf_plant, cmd, k.wx, k.wy, k.wz, ag, acmd, aw, nullptr);
            A.wx += aw[0]; A.wy += aw[1]; A.wz += aw[2];
        }
        if constexpr (MODE == GPD_CTBR_POS) {
            float gp[3], gq[4], gv[3], gt[3], gtv[3];
            if constexpr (GG)
                gpd_ctbr_outer_vjp(&B, k0.px, k0.py, k0.pz, k0.qx, k0.qy, k0.qz, k0.qw, k0.vx, k0.vy, k0.vz, row.a.x, row.a.y, row.a.z, row.b.z,
                                   row.b.w, row.c.x, acmd, gp, gq, gv, gt, gtv, gk);
            else
                gpd_ctbr_outer_vjp(&B, k0.px, k0.py, k0.pz, k0.qx, k0.qy, k0.qz, k0.qw, k0.vx, k0.vy, k0.vz, row.a.x, row.a.y, row.a.z, row.b.z,
                                   row.b.w, row.c.x, acmd, gp, gq, gv, gt, gtv, nullptr);
            A.px += gp[0]; A.py += gp[1]; A.pz += gp[2];
            A.qx += gq[0]; A.qy += gq[1]; A.qz += gq[2]; A.qw += gq[3];
            A.vx += gv[0]; A.vy += gv[1]; A.vz += gv[2];
            // the target row's gradient: pos | rpy (ignored: exact zeros) | vel | rpy rates (zeros)
            f4v* dst = reinterpret_cast<f4v*>(g_rows + (static_cast<size_t>(t) * N + n) * 12);
            dst[0] = f4v{gt[0], gt[1], gt[2], 0.0f};
            dst[1] = f4v{0.0f, 0.0f, gtv[0], gtv[1]};
            dst[2] = f4v{gtv[2], 0.0f, 0.0f, 0.0f};
        } else {
            *reinterpret_cast<f4v*>(g_rows + (static_cast<size_t>(t) * N + n) * 4) = f4v{acmd[0], acmd[1], acmd[2], acmd[3]};
        }
    }
    kin_store(g_kin, ld, n, A);
    if constexpr (GG) {
        const uint32_t off4 = n * 4u;
        st_row(g_gains, ld, 0, off4, gk[0]); st_row(g_gains, ld, 1, off4, gk[1]); st_row(g_gains, ld, 2, off4, gk[2]);
        st_row(g_gains, ld, 3, off4, gk[3]); st_row(g_gains, ld, 4, off4, gk[4]); st_row(g_gains, ld, 5, off4, gk[5]);
        st_row(g_gains, ld, 6, off4, gk[6]); st_row(g_gains, ld, 7, off4, gk[7]); st_row(g_gains, ld, 8, off4, gk[8]);
        st_row(g_gains, ld, 9, off4, gr[0]); st_row(g_gains, ld, 10, off4, gr[1]); st_row(g_gains, ld, 11, off4, gr[2]);
    } else {
        (void)g_gains; (void)gk; (void)gr;
    }
}

// [a, a + na) and [b, b + nb) floats share a word (NULL shares nothing)
bool ctbr_overlap(const float* a, int64_t na, const float* b, int64_t nb) { return a && b && a < b + nb && b < a + na; }

// MODE x PLANT: both kernels of this file are launched as launch(mode, plant)
template <class F>
void diff_ctbr_dispatch(int32_t mode, bool plant, F&& launch) {
    with_ext_plant(false, plant, [&](auto, auto pl) {
        if (mode == GPD_CTBR_POS) launch(Const<GPD_CTBR_POS>{}, pl); else launch(Const<GPD_CTBR_CMD>{}, pl);
    });
}

// what both entries check of mode, the strides and the row block, after the configuration
int ctbr_rows_check(Refuse bad, int32_t mode, int64_t N, int64_t row_step_stride, int64_t obs_step_stride) {
    const int64_t width = mode == GPD_CTBR_POS ? 12 : 4;
    if ((row_step_stride != 0 && row_step_stride < width * N) || (obs_step_stride != 0 && obs_step_stride < 12 * N))
        return bad(GPD_EINVAL, "a non-zero step stride must cover a step's rows (4*num_envs commands or 12*num_envs targets; 12*num_envs for obs12)");
    if ((row_step_stride & 3) || (obs_step_stride & 3)) return bad(GPD_EINVAL, "step strides must be multiples of 4 floats (16-byte rows)");
    return 0;
}

}  // namespace

extern "C" {

int gpd_rollout_tape_ctbr_floats(const GpdStepCfg* cfg, int32_t num_steps, int64_t ld, int64_t* floats_out) {
    // 13 kinematic floats per control step
    return tape_floats_impl(Refuse{"gpd_rollout_tape_ctbr_floats"}, DiffFamily::CTBR, cfg, num_steps, ld, 13, 0, floats_out);
}

int gpd_rollout_tape_ctbr(const GpdParams* params, const GpdCtbr* ctbr, const GpdState* state, const GpdStepCfg* cfg, int32_t mode,
                          const float* rows, int64_t row_step_stride, const float* plant_rows, float* obs12, int64_t obs_step_stride,
                          float* cmd_out, int32_t num_steps, float* tape, void* stream) {
    const Refuse bad{"gpd_rollout_tape_ctbr"};
    if (!params || !ctbr || !state || !cfg) return bad(GPD_EINVAL, "NULL params/ctbr/state/cfg");
    if (int rc = check_state(bad, state)) return rc;
    if (!rows || !obs12 || !tape) return bad(GPD_EINVAL, "NULL rows/obs12/tape");
    if (mode != GPD_CTBR_CMD && mode != GPD_CTBR_POS) return bad(GPD_EINVAL, "unknown mode (GPD_CTBR_CMD or GPD_CTBR_POS)");
    if (int rc = diff_cfg(bad, DiffFamily::CTBR, cfg, state->ld, num_steps, row_step_stride, obs_step_stride)) return rc;
    if (state->dw_force) return bad(GPD_ENOTSUP, "state.dw_force (downwash needs mates) is not differentiable");
    if (int rc = check_needs(bad, params, state, cfg, nullptr, nullptr)) return rc;
    const int64_t N = cfg->num_envs;
    if (int rc = ctbr_rows_check(bad, mode, N, row_step_stride, obs_step_stride)) return rc;
    if (misaligned16(rows) || misaligned16(obs12) || misaligned16(plant_rows) || misaligned16(cmd_out) || misaligned16(tape))
        return bad(GPD_EINVAL, "rows, obs12, plant_rows, cmd_out and tape must be 16-byte aligned");
    if (cmd_out && cmd_out == rows) return bad(GPD_EINVAL, "cmd_out must not alias rows");
    if (!(cfg->ctrl_dt > 0.0f) || !(cfg->pyb_dt > 0.0f)) return bad(GPD_EINVAL, "pyb_dt and ctrl_dt must be positive");
    GpdStepCfg C = *cfg;
    C.target_per_env = 0; C.init_per_env = 0;
    const int64_t cmd_stride = mode == GPD_CTBR_POS ? 4 * N : row_step_stride;
    const dim3 grid(blocks_for(N, kBlock));
    diff_ctbr_dispatch(mode, plant_rows != nullptr, [&](auto mode_, auto plant_) {
        hipLaunchKernelGGL((gpd_rollout_tape_ctbr_kernel<decltype(mode_)::value, decltype(plant_)::value>), grid, dim3(kBlock), 0,
                           static_cast<hipStream_t>(stream), *params, *ctbr, state->kin, state->last_rpm, state->step_counter, state->bad,
                           static_cast<uint32_t>(state->ld), C, rows, row_step_stride, plant_rows, obs12, obs_step_stride, cmd_out, cmd_stride,
                           num_steps, tape);
    });
    return launched(bad.who);
}

int gpd_rollout_vjp_ctbr(const GpdParams* params, const GpdCtbr* ctbr, const GpdStepCfg* cfg, int64_t ld, int32_t mode, int32_t num_steps,
                         const float* rows, int64_t row_step_stride, const float* plant_rows, const float* tape, const float* g_obs12,
                         int64_t obs_step_stride, float* g_kin, float* g_rows, float* g_gains, void* stream) {
    const Refuse bad{"gpd_rollout_vjp_ctbr"};
    if (!params || !ctbr || !cfg) return bad(GPD_EINVAL, "NULL params/ctbr/cfg");
    if (!rows || !tape || !g_kin || !g_rows) return bad(GPD_EINVAL, "NULL rows/tape/g_kin/g_rows");
    if (mode != GPD_CTBR_CMD && mode != GPD_CTBR_POS) return bad(GPD_EINVAL, "unknown mode (GPD_CTBR_CMD or GPD_CTBR_POS)");
    if (int rc = sweep_prologue(bad, DiffFamily::CTBR, params, cfg, ld, num_steps, row_step_stride, obs_step_stride, 0, nullptr, tape, g_kin))
        return rc;
    const int64_t N = cfg->num_envs, width = mode == GPD_CTBR_POS ? 12 : 4;
    if (int rc = ctbr_rows_check(bad, mode, N, row_step_stride, obs_step_stride)) return rc;
    if (misaligned16(rows) || misaligned16(plant_rows) || misaligned16(g_obs12) || misaligned16(g_rows) || misaligned16(g_gains))
        return bad(GPD_EINVAL, "rows, plant_rows, g_obs12, g_rows and g_gains must be 16-byte aligned");
    if (13 * static_cast<int64_t>(num_steps) > INT64_MAX / ld) return bad(GPD_ERANGE, "the tape does not fit 2^63 floats");
    const int64_t n_kin = 13 * ld, n_tape = 13 * ld * num_steps, n_rows = width * N * num_steps, n_gains = 12 * ld;
    if (ctbr_overlap(g_rows, n_rows, g_gains, n_gains) || ctbr_overlap(g_rows, n_rows, g_kin, n_kin) || ctbr_overlap(g_gains, n_gains, g_kin, n_kin) ||
        ctbr_overlap(g_rows, n_rows, tape, n_tape) || ctbr_overlap(g_gains, n_gains, tape, n_tape) || ctbr_overlap(g_kin, n_kin, tape, n_tape))
        return bad(GPD_EINVAL, "g_rows, g_gains, g_kin and tape must not alias one another");
    const dim3 grid(blocks_for(N, kBlock));
    diff_ctbr_dispatch(mode, plant_rows != nullptr, [&](auto mode_, auto plant_) {
        auto launch = [&](auto gg) {
            hipLaunchKernelGGL((gpd_rollout_vjp_ctbr_kernel<decltype(mode_)::value, decltype(plant_)::value, decltype(gg)::value>), grid,
                               dim3(kBlock), 0, static_cast<hipStream_t>(stream), *params, *ctbr, *cfg, ld, num_steps, rows, row_step_stride,
                               plant_rows, tape, g_obs12, obs_step_stride, g_kin, g_rows, g_gains);
        };
        if (g_gains) launch(Const<true>{}); else launch(Const<false>{});
    });
    return launched(bad.who);
}

}  // extern "C"
