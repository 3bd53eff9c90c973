// mppi_peers.inc -- gpd_mppi_peers (include/gpd.h): gpd_mppi / gpd_mppi_ctbr with one more term in the running cost, a hinge on the
// distance to where each of up to 32 PEERS will be after the step (rows of a table [H][n_rows][4] that the peers published), and one
// more output, path_out: where this drone now plans to be, which its peers read in turn.  Pulled into abi.hip behind mppi_ctbr.inc:
// the action and the butterflies are mppi.inc's, the state cost and the update mppi_ctbr.inc's device helpers, the peer's hinge
// mppi_peers_math.inc.  gpd_mppi_kernel and gpd_mppi_ctbr_kernel are left textually as they are.  DESIGN.md section 3.20.
//
// The house shape: one wave per drone, lane = sample, pass 1 / butterflies / pass 2 (mppi_update), no atomics, no LDS, one writer per
// word.  A drone's peers are the same for all its samples, so they are fetched once per step and WAVE: lane j < k keeps idx[n][j] in a
// register for the whole kernel (-1 for an entry that is skipped) and loads its peer's 16-byte row of the step -- the row of the NEXT
// step is requested before the model's arithmetic of this one -- and a uniform loop over j hands x, y, z to every lane with
// v_readlane at a uniform j.  A skipped entry's row is NaN, which the hinge answers with exactly 0 and the nearest distance does not
// count: no divergence in the loop, and the sum is the one over the counted entries in their order.
// path_out: after the update the wave flies u_out -- as lane 0 stored it -- once more without noise, every lane the same arithmetic,
// and lane 0 stores the position after each step and the distance to the nearest counted peer there.
#include "mppi_peers_math.inc"

namespace {

constexpr int kPeersCtbr = -1;                    // the ACT of the CTBR model (the others: GPD_ACT_RPM, GPD_ACT_VEL)

__device__ __forceinline__ float lane_value(float v, int j) {
    return __builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, v), j));
}

// one step of the model on the action a: gpd_mppi_kernel's (RPM, VEL) or gpd_mppi_ctbr_kernel's (CTBR), the same statements
template <int ACT>
__device__ __forceinline__ void peers_model_step(const GpdParams& P, const GpdCtbr& B, const GpdStepCfg& C, const float4 a, Carry& c) {
    Kin& k = c.k;
    float d0, d1, d2;
    if constexpr (ACT == kPeersCtbr) {
        const float cmd[4] = {a.x, a.y, a.z, a.w};
        for (int ss = 0; ss < C.substeps; ++ss) {
            float rpm[4], g[4];
            gpd_ctbr_rate_loop(&B, P.M, P.J[0], P.J[1], P.J[2], cmd, k.wx, k.wy, k.wz, rpm);
#pragma unroll
            for (int i = 0; i < 4; ++i) g[i] = thrust_dev(P, rpm[i]);
            substep<false, false>(P, C.pyb_dt, 0u, g, 0.0f, 0.0f, k, d0, d1, d2);
        }
    } else {
        constexpr bool PID = ACT == GPD_ACT_VEL;
        float rpm[4], g[4];
        map_action<PID, 4, ACT>(P, C, a, c, rpm, g);
        for (int ss = 0; ss < C.substeps; ++ss) substep<false, false>(P, C.pyb_dt, 0u, g, 0.0f, 0.0f, k, d0, d1, d2);
        if constexpr (PID) quat_to_rpy(k.qx, k.qy, k.qz, k.qw, c.roll, c.pitch, c.yaw);
    }
}

// the sum of the hinges of the point (px, py, pz) against the step's rows (lane j holds entry j's; NaN: skipped), j = 0 .. k-1 in that
// order; NEAR: `nearest` becomes the distance to the nearest counted one (GPD_OBST_INF: none)
template <bool NEAR>
__device__ __forceinline__ float peers_sum(const float4 row, const int k, const float peer_dist, const float px, const float py, const float pz,
                                           float& nearest) {
    float sum = 0.0f;
    if constexpr (NEAR) nearest = GPD_OBST_INF;
    for (int j = 0; j < k; ++j) {
        const float dx = px - lane_value(row.x, j), dy = py - lane_value(row.y, j), dz = pz - lane_value(row.z, j);
        sum += gpd_mppi_peer_pen(peer_dist, dx, dy, dz);
        if constexpr (NEAR) nearest = gpd_mppi_peer_nearest(gpd_mppi_peer_distance(dx, dy, dz), nearest);
    }
    return sum;
}

// ACT: GPD_ACT_RPM, GPD_ACT_VEL or kPeersCtbr; OBST: a list is given
template <int ACT, bool OBST>
__global__ __launch_bounds__(kBlock) void gpd_mppi_peers_kernel(const GpdParams P, const GpdCtbr B, const GpdStepCfg C, const GpdMppi Q, const GpdMppiPeers R,
                                                                const float* __restrict__ kin, const float* __restrict__ pid, const int64_t ld,
                                                                const int N, const float* __restrict__ u_in, const int64_t u_stride,
                                                                const float* __restrict__ goal, const int64_t goal_stride,
                                                                const float* __restrict__ obst, const int n_obst, const int64_t obst_ld,
                                                                float* __restrict__ u_out, float* __restrict__ costs, float4* __restrict__ stats4) {
    constexpr bool PID = ACT == GPD_ACT_VEL;
    const int wave = __builtin_amdgcn_readfirstlane(static_cast<int>(threadIdx.x) >> 6);
    const int n = static_cast<int>(blockIdx.x) * kMppiDrones + wave;          // this wave's drone: uniform
    if (n >= N) return;
    const uint32_t lane = threadIdx.x & 63u;
    const int H = Q.horizon, batches = Q.samples >> 6;

    // ---- what the samples share, uniform: the start state (and the controller members), the nominal, the goal, the list ----
    const float4 kp = kin_P(kin, ld)[n], kq = kin_Q(kin, ld)[n], kv = kin_V(kin, ld)[n];
    const float kwz = kin[12 * ld + n];
    Carry c0;
    c0.k = Kin{kp.x, kp.y, kp.z, kq.x, kq.y, kq.z, kq.w, kv.x, kv.y, kv.z, kp.w, kv.w, kwz};
    c0.s = Pid{0, 0, 0, 0, 0, 0, 0, 0, 0};
    c0.l0 = c0.l1 = c0.l2 = c0.l3 = 0.0f; c0.counter = 0; c0.dw_in = 0.0f;
    c0.roll = c0.pitch = c0.yaw = 0.0f;
    if constexpr (PID) {
        c0.s.ipx = pid[0 * ld + n]; c0.s.ipy = pid[1 * ld + n]; c0.s.ipz = pid[2 * ld + n];
        c0.s.lr = pid[3 * ld + n]; c0.s.lp = pid[4 * ld + n]; c0.s.ly = pid[5 * ld + n];
        c0.s.irx = pid[6 * ld + n]; c0.s.iry = pid[7 * ld + n]; c0.s.irz = pid[8 * ld + n];
        quat_to_rpy(kq.x, kq.y, kq.z, kq.w, c0.roll, c0.pitch, c0.yaw);
    }
    const float* const un = u_in + static_cast<int64_t>(n) * 4;
    const float* const gn = goal + static_cast<int64_t>(n) * 4;
    const int64_t opitch = obst_ld == 0 ? 1 : obst_ld;
    const float* const ob = OBST ? obst + (obst_ld == 0 ? 0 : n) : nullptr;
    float* const cn = costs + static_cast<int64_t>(n) * Q.samples;

    // ---- this lane's peer: entry `lane` of the drone's row of idx, kept for the whole kernel; counted if it names another row of pos ----
    const int k = R.k;
    int pj = -1;
    if (lane < static_cast<uint32_t>(k)) pj = R.idx[static_cast<int64_t>(n) * R.idx_ld + lane];
    const bool counted = pj >= 0 && pj < R.n_rows && pj != n;
    const float* const prow = R.pos + static_cast<int64_t>(counted ? pj : 0) * 4;
    const float none = __builtin_nanf("");
    auto peer_row = [&](const int h) {        // the lane's peer after step h
        return counted ? *reinterpret_cast<const float4*>(prow + h * R.pos_step_stride) : make_float4(none, none, none, none);
    };
    float unused;

    // ---- pass 1: the samples' costs ----
    for (int b = 0; b < batches; ++b) {
        const uint32_t m = static_cast<uint32_t>(b) * 64u + lane;
        Carry c = c0;
        float S = 0.0f;
        float4 next = peer_row(0);
        for (int h = 0; h < H; ++h) {
            const float4 row = next;
            if (h + 1 < H) next = peer_row(h + 1);
            const float4 u = *reinterpret_cast<const float4*>(un + h * u_stride);
            const float4 g4 = *reinterpret_cast<const float4*>(gn + h * goal_stride);
            const float4 a = mppi_action(Q, static_cast<uint32_t>(n), m, static_cast<uint32_t>(h), u);
            peers_model_step<ACT>(P, B, C, a, c);
            const float cost = mppi_state_cost<OBST>(Q, c.k, g4, h == H - 1, ob, opitch, n_obst);
            S += cost + R.w_peer * peers_sum<false>(row, k, R.peer_dist, c.k.px, c.k.py, c.k.pz, unused);
        }
        cn[m] = S;
    }
    float* const on = u_out + static_cast<int64_t>(n) * 4;
    mppi_update(Q, n, lane, cn, un, u_stride, on, stats4);

    // ---- the path of the new nominal: u_out as lane 0 stored it (the same wave reads it back: in order), flown without noise ----
    if (R.path_out == nullptr) return;
    __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront");
    float* const pn = R.path_out + static_cast<int64_t>(n) * 4;
    Carry c = c0;
    float4 next = peer_row(0);
    for (int h = 0; h < H; ++h) {
        const float4 row = next;
        if (h + 1 < H) next = peer_row(h + 1);
        const f4v u = *reinterpret_cast<const f4v*>(on + h * u_stride);
        peers_model_step<ACT>(P, B, C, make_float4(u.x, u.y, u.z, u.w), c);
        float nearest;
        (void)peers_sum<true>(row, k, R.peer_dist, c.k.px, c.k.py, c.k.pz, nearest);
        const f4v out = {c.k.px, c.k.py, c.k.pz, nearest};
        if (lane == 0) *reinterpret_cast<f4v*>(pn + h * u_stride) = out;
    }
}

}  // namespace

extern "C" int gpd_mppi_peers(const GpdParams* params, const GpdCtbr* ctbr, const GpdState* state, const GpdStepCfg* cfg, const GpdMppi* mppi,
                              const GpdMppiPeers* peers, const float* u_in, int64_t u_step_stride, const float* goal, int64_t goal_step_stride,
                              const float* obst, int32_t n_obst, int64_t obst_ld, float* u_out, float* costs, float* stats4, void* stream) {
    const Refuse bad{"gpd_mppi_peers"};
    if (!params || !state || !cfg || !mppi || !peers) return bad(GPD_EINVAL, "NULL params/state/cfg/mppi/peers");
    if (!u_in || !goal || !u_out || !costs || !stats4) return bad(GPD_EINVAL, "NULL u_in/goal/u_out/costs/stats4");
    if (!peers->idx || !peers->pos) return bad(GPD_EINVAL, "NULL peers.idx/peers.pos");
    if (int rc = check_state(bad, state)) return rc;
    if (int rc = check_ranges(bad, cfg)) return rc;
    if (int rc = check_positive(bad, cfg)) return rc;
    if (int rc = check_flags(bad, cfg)) return rc;
    const int64_t N = static_cast<int64_t>(cfg->num_envs) * cfg->drones_per_env;
    if (int rc = check_extent(bad, N, state->ld)) return rc;
    // what the planning model is: gpd_mppi's (ctbr NULL) or gpd_mppi_ctbr's
    if (cfg->drones_per_env != 1) return bad(GPD_ENOTSUP, "aviaries of more than one drone are not planned for (drones_per_env must be 1)");
    if (cfg->physics_flags != 0u) return bad(GPD_ENOTSUP, "the planning model has no physics_flags (drag, ground effect, downwash, ground plane, damping)");
    if (cfg->task != GPD_TASK_NONE || cfg->auto_reset) return bad(GPD_ENOTSUP, "the planning model has no episode ends (task must be GPD_TASK_NONE, auto_reset 0)");
    if (ctbr != nullptr) {
        if (cfg->act_type != GPD_ACT_RAW_RPM && cfg->act_type != GPD_ACT_DIRECT_RPM)
            return bad(GPD_ENOTSUP, "with ctbr, act_type GPD_ACT_RAW_RPM or GPD_ACT_DIRECT_RPM (the rate loop's output is RPMs)");
    } else {
        if (cfg->act_type != GPD_ACT_RPM && cfg->act_type != GPD_ACT_VEL) return bad(GPD_ENOTSUP, "without ctbr, act_type must be GPD_ACT_RPM or GPD_ACT_VEL");
        if (int rc = check_needs(bad, params, state, cfg, nullptr, nullptr)) return rc;
    }
    const GpdMppi& q = *mppi;
    if (int rc = check_mppi_plan(bad, q, N, u_in, u_step_stride, goal, goal_step_stride, obst, n_obst, obst_ld, u_out, stats4)) return rc;
    const GpdMppiPeers& r = *peers;
    if (r.k < 1 || r.k > 32) return bad(GPD_EINVAL, "peers.k must be in 1..32");
    if (r.idx_ld < r.k) return bad(GPD_EINVAL, "peers.idx_ld must be >= peers.k");
    if (r.n_rows < N) return bad(GPD_EINVAL, "peers.n_rows must be >= num_envs (rows 0 .. N-1 of pos are the planned drones)");
    if (r.pos_step_stride != 0 && (r.pos_step_stride % 4 != 0 || r.pos_step_stride < 4 * static_cast<int64_t>(r.n_rows)))
        return bad(GPD_EINVAL, "peers.pos_step_stride must be 0 or a multiple of 4 floats >= 4 * peers.n_rows");
    if (misaligned16(r.pos) || misaligned16(r.path_out)) return bad(GPD_EINVAL, "peers.pos and peers.path_out must be 16-byte aligned");
    if (r.path_out != nullptr && (r.path_out == u_in || r.path_out == u_out)) return bad(GPD_EINVAL, "peers.path_out must not alias u_in or u_out");
    if (!(r.w_peer >= 0.0f) || !(r.w_peer < GPD_OBST_INF) || !(r.peer_dist >= 0.0f) || !(r.peer_dist < GPD_OBST_INF))
        return bad(GPD_EINVAL, "peers.w_peer and peers.peer_dist must be non-negative and finite");
    const bool has_obst = obst != nullptr && n_obst > 0;
    const GpdCtbr no_ctbr{};
    auto launch = [&](auto act, auto ob) {
        hipLaunchKernelGGL((gpd_mppi_peers_kernel<decltype(act)::value, decltype(ob)::value>), dim3(blocks_for(N, kMppiDrones)), dim3(kBlock), 0,
                           static_cast<hipStream_t>(stream), *params, ctbr != nullptr ? *ctbr : no_ctbr, *cfg, q, r, state->kin, state->pid, state->ld,
                           static_cast<int>(N), u_in, u_step_stride, goal, goal_step_stride, obst, n_obst, obst_ld, u_out, costs,
                           reinterpret_cast<float4*>(stats4));
    };
    auto with_obst = [&](auto act) { if (has_obst) launch(act, Const<true>{}); else launch(act, Const<false>{}); };
    if (ctbr != nullptr) with_obst(Const<kPeersCtbr>{});
    else if (cfg->act_type == GPD_ACT_VEL) with_obst(Const<static_cast<int>(GPD_ACT_VEL)>{});
    else with_obst(Const<static_cast<int>(GPD_ACT_RPM)>{});
    return launched(bad.who);
}
