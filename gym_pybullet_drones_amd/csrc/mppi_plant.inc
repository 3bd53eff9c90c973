// mppi_plant.inc -- gpd_mppi_plant (include/gpd.h): gpd_mppi (ctbr NULL) or gpd_mppi_ctbr (ctbr given) on the aviary's own model -- every
// drone's row of the plant table (gpd_plant_derive; the airframe gpd_rollout_plant flies) and the force terms of cfg.physics_flags
// (ground effect, drag, the ground plane, Bullet's damping) in the model step.  Pulled into abi.hip behind mppi_peers.inc: the action
// and the butterflies are mppi.inc's, the state cost and the update mppi_ctbr.inc's device helpers, the sub-step, the action mapping
// and the plant copy gpd_common.inc's, the rate loop ctbr_math.inc's.  gpd_mppi_kernel, gpd_mppi_ctbr_kernel and gpd_mppi_peers_kernel
// are left textually as they are.  DESIGN.md section 3.21.
//
// The house shape: one wave per drone, lane = sample, pass 1 / butterflies / pass 2 (mppi_update), no atomics, no LDS, one writer per
// word.  One wave is one drone, so the drone's plant row is WAVE-UNIFORM: its 19 floats are read once, before pass 1, at uniform
// addresses (rows[r * ld + n], n uniform) over a copy of the nominal struct, as plant_of<true> overwrites them by name -- the airframe
// sits in scalar registers next to the nominal one, where the rollout's plant path (one drone per LANE) pays 19 VGPRs.  The last RPMs
// (the drag term's "previous action") are read the same way and then carried per sample.

namespace {

constexpr int kPlantCtbr = kPeersCtbr;            // the ACT of the CTBR model (the others: GPD_ACT_RPM, GPD_ACT_VEL)

// One step of the model on the action a.  RPM, VEL: env_step's for one drone -- map_action on the plant type, the sub-steps (the drag
// term sees the previous step's RPMs on the first sub-step and this step's after it), the rpy refresh, the RPMs carried.  CTBR:
// gpd_rollout_ctbr_kernel's -- the rate loop on the nominal M and J, thrust_dev and the sub-step on the plant, the drag term on the
// RPMs applied one sub-step earlier.  Without EXT and on GpdParams these are gpd_mppi_kernel's / gpd_mppi_ctbr_kernel's statements.
template <int ACT, bool EXT, class PP>
__device__ __forceinline__ void plant_model_step(const GpdParams& P, const PP& A, const GpdCtbr& B, const GpdStepCfg& C, const uint32_t flags,
                                                 const float4 a, Carry& c) {
    Kin& k = c.k;
    const bool drag = EXT && (flags & GPD_PHYS_DRAG);
    float d0, d1, d2;
    if constexpr (ACT == kPlantCtbr) {
        const float cmd[4] = {a.x, a.y, a.z, a.w};
        for (int ss = 0; ss < C.substeps; ++ss) {
            float rpm[4], g[4];
            gpd_ctbr_rate_loop(&B, P.M, P.J[0], P.J[1], P.J[2], cmd, k.wx, k.wy, k.wz, rpm);
#pragma unroll
            for (int i = 0; i < 4; ++i) g[i] = thrust_dev(A, rpm[i]);
            const float drag_sum = drag ? ((c.l0 + c.l1) + c.l2) + c.l3 : 0.0f;
            substep<EXT, false>(A, C.pyb_dt, flags, g, drag_sum, 0.0f, k, d0, d1, d2);
            if constexpr (EXT) { c.l0 = rpm[0]; c.l1 = rpm[1]; c.l2 = rpm[2]; c.l3 = rpm[3]; }
        }
    } else {
        constexpr bool PID = ACT == GPD_ACT_VEL;
        float rpm[4], g[4];
        map_action<PID, 4, ACT>(A, C, a, c, rpm, g);
        const float cur_sum = ((rpm[0] + rpm[1]) + rpm[2]) + rpm[3];
        float drag_sum = drag ? ((c.l0 + c.l1) + c.l2) + c.l3 : 0.0f;
        for (int ss = 0; ss < C.substeps; ++ss) {
            substep<EXT, false>(A, C.pyb_dt, flags, g, drag_sum, 0.0f, k, d0, d1, d2);
            drag_sum = drag ? cur_sum : 0.0f;
        }
        if constexpr (PID) quat_to_rpy(k.qx, k.qy, k.qz, k.qw, c.roll, c.pitch, c.yaw);
        if constexpr (EXT) { c.l0 = rpm[0]; c.l1 = rpm[1]; c.l2 = rpm[2]; c.l3 = rpm[3]; }
    }
}

// ACT: GPD_ACT_RPM, GPD_ACT_VEL or kPlantCtbr; OBST: a list is given; EXT: some physics flag is set (`flags` is cfg.physics_flags at run
// time); PLANT: a table is given
template <int ACT, bool OBST, bool EXT, bool PLANT>
__global__ __launch_bounds__(kBlock) void gpd_mppi_plant_kernel(const GpdParams P, const GpdCtbr B, const GpdStepCfg C, const GpdMppi Q,
                                                                const float* __restrict__ kin, const float* __restrict__ pid,
                                                                const float* __restrict__ last_rpm, const float* __restrict__ plant,
                                                                const int64_t ld, const int N, const float* __restrict__ u_in,
                                                                const int64_t u_stride, const float* __restrict__ goal, const int64_t goal_stride,
                                                                const float* __restrict__ obst, const int n_obst, const int64_t obst_ld,
                                                                float* __restrict__ u_out, float* __restrict__ costs, float4* __restrict__ stats4) {
    constexpr bool PID = ACT == GPD_ACT_VEL;
    const int wave = __builtin_amdgcn_readfirstlane(static_cast<int>(threadIdx.x) >> 6);
    const int n = static_cast<int>(blockIdx.x) * kMppiDrones + wave;          // this wave's drone: uniform
    if (n >= N) return;
    const uint32_t lane = threadIdx.x & 63u;
    const int H = Q.horizon, batches = Q.samples >> 6;
    const uint32_t flags = EXT ? C.physics_flags : 0u;

    // ---- what the samples share, uniform: the drone's airframe, the start state (the controller members, the last RPMs) ----
    std::conditional_t<PLANT, PlantParams, GpdParams> A = plant_of<PLANT>(P, plant, ld, static_cast<uint32_t>(n) * 4u);
    // (the rotor offsets of the ground effect, and the three neighbours of the host-only word pid_kf, as opaque scalars: fetched as
    // parts of overlapping multi-word scalar loads they are otherwise kept in VGPR lanes as tuples of which one register was reused,
    // the shape tests/test_kernel_isa.py refuses in every kernel of the library; no arithmetic changes)
    if constexpr (EXT)
        asm volatile("" : "+s"(A.prop_x[0]), "+s"(A.prop_x[1]), "+s"(A.prop_x[2]), "+s"(A.prop_x[3]), "+s"(A.prop_y[0]), "+s"(A.prop_y[1]),
                          "+s"(A.prop_y[2]), "+s"(A.prop_y[3]));
    if constexpr (PID) asm volatile("" : "+s"(A.hover_resid), "+s"(A.km_over_kf), "+s"(A.pid_gravity));
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
    if constexpr (EXT) {
        if (flags & GPD_PHYS_DRAG) {           // (the entry refuses the flag without state.last_rpm)
            c0.l0 = last_rpm[0 * ld + n]; c0.l1 = last_rpm[1 * ld + n]; c0.l2 = last_rpm[2 * ld + n]; c0.l3 = last_rpm[3 * ld + n];
        }
    }
    const float* const un = u_in + static_cast<int64_t>(n) * 4;
    const float* const gn = goal + static_cast<int64_t>(n) * 4;
    const int64_t opitch = obst_ld == 0 ? 1 : obst_ld;
    const float* const ob = OBST ? obst + (obst_ld == 0 ? 0 : n) : nullptr;
    float* const cn = costs + static_cast<int64_t>(n) * Q.samples;

    // ---- pass 1: the samples' costs ----
    for (int b = 0; b < batches; ++b) {
        const uint32_t m = static_cast<uint32_t>(b) * 64u + lane;
        Carry c = c0;
        float S = 0.0f;
        for (int h = 0; h < H; ++h) {
            const float4 u = *reinterpret_cast<const float4*>(un + h * u_stride);
            const float4 g4 = *reinterpret_cast<const float4*>(gn + h * goal_stride);
            const float4 a = mppi_action(Q, static_cast<uint32_t>(n), m, static_cast<uint32_t>(h), u);
            plant_model_step<ACT, EXT>(P, A, B, C, flags, a, c);
            S += mppi_state_cost<OBST>(Q, c.k, g4, h == H - 1, ob, opitch, n_obst);
        }
        cn[m] = S;
    }
    mppi_update(Q, n, lane, cn, un, u_stride, u_out + static_cast<int64_t>(n) * 4, stats4);
}

}  // namespace

extern "C" int gpd_mppi_plant(const GpdParams* params, const GpdCtbr* ctbr, const GpdState* state, const GpdStepCfg* cfg, const GpdMppi* mppi,
                              const float* plant_rows, const float* u_in, int64_t u_step_stride, const float* goal, int64_t goal_step_stride,
                              const float* obst, int32_t n_obst, int64_t obst_ld, float* u_out, float* costs, float* stats4, void* stream) {
    const Refuse bad{"gpd_mppi_plant"};
    if (!params || !state || !cfg || !mppi) return bad(GPD_EINVAL, "NULL params/state/cfg/mppi");
    if (!u_in || !goal || !u_out || !costs || !stats4) return bad(GPD_EINVAL, "NULL u_in/goal/u_out/costs/stats4");
    if (int rc = check_state(bad, state)) return rc;
    if (int rc = check_ranges(bad, cfg)) return rc;
    if (int rc = check_positive(bad, cfg)) return rc;
    if (int rc = check_flags(bad, cfg)) return rc;
    const int64_t N = static_cast<int64_t>(cfg->num_envs) * cfg->drones_per_env;
    if (int rc = check_extent(bad, N, state->ld)) return rc;
    // what the planning model is: gpd_mppi's (ctbr NULL) or gpd_mppi_ctbr's, with the force terms a single drone has
    if (cfg->drones_per_env != 1) return bad(GPD_ENOTSUP, "aviaries of more than one drone are not planned for (drones_per_env must be 1)");
    if ((cfg->physics_flags & GPD_PHYS_DW) || state->dw_force) return bad(GPD_ENOTSUP, "the planning model has no downwash (it needs mates)");
    if (cfg->task != GPD_TASK_NONE || cfg->auto_reset) return bad(GPD_ENOTSUP, "the planning model has no episode ends (task must be GPD_TASK_NONE, auto_reset 0)");
    if (ctbr != nullptr) {
        if (cfg->act_type != GPD_ACT_RAW_RPM && cfg->act_type != GPD_ACT_DIRECT_RPM)
            return bad(GPD_ENOTSUP, "with ctbr, act_type GPD_ACT_RAW_RPM or GPD_ACT_DIRECT_RPM (the rate loop's output is RPMs)");
    } else {
        if (cfg->act_type != GPD_ACT_RPM && cfg->act_type != GPD_ACT_VEL) return bad(GPD_ENOTSUP, "without ctbr, act_type must be GPD_ACT_RPM or GPD_ACT_VEL");
    }
    if (int rc = check_needs(bad, params, state, cfg, nullptr, nullptr)) return rc;
    const GpdMppi& q = *mppi;
    if (int rc = check_mppi_plan(bad, q, N, u_in, u_step_stride, goal, goal_step_stride, obst, n_obst, obst_ld, u_out, stats4)) return rc;
    if (misaligned16(plant_rows)) return bad(GPD_EINVAL, "plant_rows must be 16-byte aligned");
    const bool has_obst = obst != nullptr && n_obst > 0;
    const bool ext = (cfg->physics_flags & 31u) != 0;
    const GpdCtbr no_ctbr{};
    auto launch = [&](auto act, auto ob) {
        with_ext_plant(ext, plant_rows != nullptr, [&](auto ext_, auto plant_) {
            hipLaunchKernelGGL((gpd_mppi_plant_kernel<decltype(act)::value, decltype(ob)::value, decltype(ext_)::value, decltype(plant_)::value>),
                               dim3(blocks_for(N, kMppiDrones)), dim3(kBlock), 0, static_cast<hipStream_t>(stream), *params,
                               ctbr != nullptr ? *ctbr : no_ctbr, *cfg, q, state->kin, state->pid, state->last_rpm, plant_rows, state->ld,
                               static_cast<int>(N), u_in, u_step_stride, goal, goal_step_stride, obst, n_obst, obst_ld, u_out, costs,
                               reinterpret_cast<float4*>(stats4));
        });
    };
    auto with_obst = [&](auto act) { if (has_obst) launch(act, Const<true>{}); else launch(act, Const<false>{}); };
    if (ctbr != nullptr) with_obst(Const<kPlantCtbr>{});
    else if (cfg->act_type == GPD_ACT_VEL) with_obst(Const<static_cast<int>(GPD_ACT_VEL)>{});
    else with_obst(Const<static_cast<int>(GPD_ACT_RPM)>{});
    return launched(bad.who);
}
