// rollout1_kernel_body.inc -- the body of gpd_rollout1_kernel and gpd_rollout1_plant_kernel (step_rollout.hip), included INSIDE both __global__ functions.
// A textual body rather than a __device__ function on purpose: the kernels that existed before the plant path must compile to the same
// assembly, and a body called through a function (even always inlined, its LDS arrays declared in the kernels) does not -- the kernel
// argument loads lose their no-clobber annotation and the register allocation moves.  The including kernel defines PLANT (constexpr
// bool) and `plant` (the table, nullptr without one); with PLANT false, plant_of<false> is the argument struct itself.
{
    // (member by member, never a copy of the argument structs: see gpd_step_kernel)
    const GpdState S{hot_kin, S_.last_rpm, S_.pid, hot_counter, static_cast<int64_t>(hot_ld), S_.dw_force, S_.act_ring, S_.ring_pos, S_.hist_len, 0, S_.bad};
    const GpdStepCfg C{hot_num_envs, C_.drones_per_env, C_.act_type, C_.substeps, C_.physics_flags, C_.pyb_dt, C_.ctrl_dt, C_.inv_ctrl_dt,
                       C_.lanes_per_wave, C_.task, C_.xy_bound, C_.z_bound, C_.tilt_bound, C_.term_dist, C_.trunc_counter,
                       static_cast<int32_t>((hot_bits >> 2) & 1u), static_cast<int32_t>((hot_bits >> 1) & 1u), static_cast<int32_t>(hot_bits & 1u)};
    const Span T{hot_num_steps, T_.action_stride, T_.obs_stride, T_.env_stride, T_.ring};
    const int tid = threadIdx.x;
    // workgroup -> drones: the identity.  (Bit 3 of hot_bits, never set by the host, selected every XCD one contiguous eighth of the
    // drones instead: at 65 536 drones that changed nothing, 0.816 vs 0.813-0.821 us per step, round-2 A/B.  The dead branch stays
    // until the register allocation of these kernels is re-verified without it: deleting it moves that of all 180 instantiations, and
    // one of them then saves a half-overwritten argument tuple -- tests/test_kernel_isa.py)
    uint32_t bid = blockIdx.x;
    if (hot_bits & 8u) { const uint32_t per = gridDim.x >> 3; bid = (blockIdx.x & 7u) * per + (blockIdx.x >> 3); }
    const int D = MULTI ? (DC ? DC : C.drones_per_env) : 1;
    const uint32_t N = static_cast<uint32_t>(C.num_envs) * static_cast<uint32_t>(D);
    const int K = T.num_steps;
    const uint32_t flags = EXT ? (FL >= 0 ? (static_cast<uint32_t>(FL) | (HI ? C.physics_flags & ~7u : 0u)) : C.physics_flags) : 0u;
    // lane -> drone.  A wave holds W = (64 / D) D drones: WHOLE aviaries, so that an aviary's exchange never leaves its wave (64 when D
    // divides 64 -- every lane has a drone; 63 for D = 3, 60 for D = 12 ...: the last 64 - W < D lanes of the wave are "pad" lanes).  A lane
    // without a drone -- a pad lane, or a lane past the end of the batch -- is an exact CLONE: same state, same action rows, same
    // arithmetic, hence the same bits, stored to its original's addresses (a benign duplicate write instead of a branch around the
    // stores).  Whole aviaries past the end clone the first aviary of their wave (of their workgroup, when the wave has none) and are
    // self-contained: they exchange through their own LDS slots.  A pad lane clones drone (lane - W) of its wave's first aviary and
    // reads that aviary's slots (same wave: in order).
    const int wave0 = tid & ~63, lane = tid & 63;
    const int W = MULTI ? (64 / D) * D : 64;
    const uint32_t block_base = bid * static_cast<uint32_t>(4 * W);                                   // first drone of this workgroup (< N)
    const uint32_t n0 = block_base + static_cast<uint32_t>((tid >> 6) * W);                           // first drone of this wave
    const uint32_t rows = n0 < N ? ((N - n0 < static_cast<uint32_t>(W)) ? N - n0 : static_cast<uint32_t>(W)) : 0u;   // lanes of this wave that own a drone
    const uint32_t first = rows ? n0 : block_base;                                                    // the aviary this wave's clones copy
    // the drone a row r of this wave's patch belongs to (r = lane index): its own, or its original's
    auto drone_of = [&](uint32_t r) {
        if (!MULTI) return r < rows ? n0 + r : block_base;
        const uint32_t rw = static_cast<uint32_t>(W);
        return r < rows ? n0 + r : first + (r < rw ? r - (r / static_cast<uint32_t>(D)) * static_cast<uint32_t>(D) : r - rw);
    };
    Lane L;
    L.tid = tid; L.shfl = MULTI;
    L.le = MULTI ? tid / D : tid;
    L.active = static_cast<uint32_t>(lane) < rows;
    L.n = drone_of(static_cast<uint32_t>(lane));
    L.d = MULTI ? static_cast<int>(L.n % static_cast<uint32_t>(D)) : 0;
    L.base = MULTI ? wave0 + (lane < W ? (lane / D) * D : 0) : tid;
    L.env = MULTI ? L.n / static_cast<uint32_t>(D) : L.n;

    __shared__ __attribute__((aligned(16))) float sh_rows[kBlock * 12];
    __shared__ __attribute__((aligned(16))) float sh_pos[MULTI ? 4 * kBlock : 4];   // downwash: positions of the aviary's drones
    __shared__ __attribute__((aligned(16))) float sh_red[MULTI ? 4 * kBlock : 4];   // reward | distance | out-of-bounds per drone

    // loop-invariant addressing of this lane's three 16-byte chunks of its wave's 3 KiB row patch
    uint32_t goff[3];
    const char* lsrc = reinterpret_cast<const char*>(sh_rows + wave0 * 12) + lane * 16;
#pragma unroll
    for (int j = 0; j < 3; ++j) {
        const uint32_t cidx = static_cast<uint32_t>(j * 64 + lane), r = cidx / 3u, part = cidx - 3u * r;
        goff[j] = drone_of(r) * 48u + part * 16u;                     // a clone's row goes to the row of its original
    }
    const uint32_t eoff4 = L.env * 4u;

    Carry c;
    float tgx, tgy, tgz, ip[7];
    auto fetch = [&](int step) { return load_action<AW, true>(action + (step < K ? step : K - 1) * T.action_stride, L.n); };
    const float* ipose = reinterpret_cast<const float*>(reinterpret_cast<const char*>(init_pose) +
                                                        (C.init_per_env ? L.n * 28u : static_cast<uint32_t>(L.d) * 28u));
    load_carry<PID, EXT>(S, C, flags, L, target_pos, C.auto_reset ? ipose : S.kin, c, tgx, tgy, tgz, ip);
    int ring_q = 0;                                                  // RING: the slot this aviary's next action goes to
    if constexpr (RING) {
        ring_q = S.ring_pos[L.env];
        GPD_DBG(ring_q >= 0 && ring_q < S.hist_len, GPD_DBG_RING_POS, ring_q); ring_q = GPD_DBG_CLAMP(ring_q, 0, S.hist_len - 1);
    }
    asm volatile("" :: "v"(c.k.px), "v"(c.k.py), "v"(c.k.pz), "v"(c.k.qx), "v"(c.k.qy), "v"(c.k.qz), "v"(c.k.qw), "v"(c.k.vx),
                       "v"(c.k.vy), "v"(c.k.vz), "v"(c.k.wx), "v"(c.k.wy), "v"(c.k.wz), "v"(tgx), "v"(tgy), "v"(tgz),
                       "v"(c.counter), "v"(ip[0]), "v"(ip[1]), "v"(ip[2]), "v"(ip[3]), "v"(ip[4]), "v"(ip[5]), "v"(ip[6])
                 : "memory");
    if constexpr (RING) asm volatile("" :: "v"(ring_q) : "memory");
    plant_t<PLANT> Q = plant_of<PLANT>(P, plant, S.ld, L.n * 4u);     // (PLANT: the drone's row, in registers for all K steps ...)
    plant_live<PLANT>(Q);                                            // (... requested with the state, covered by the wait below)
    __builtin_amdgcn_s_waitcnt(0x0F70);                              // vmcnt(0): the loop starts with nothing pending
    // The ONLY workgroup barrier of the launch: every wave has its state in registers before any wave can reach its
    // store_carry, so a clone lane (above) has read its original's state of step 0, not of step K.
    __builtin_amdgcn_s_barrier();
    c.roll = c.pitch = c.yaw = 0.0f;
    if (PID) quat_to_rpy(c.k.qx, c.k.qy, c.k.qz, c.k.qw, c.roll, c.pitch, c.yaw);

    (void)term_obs12;   // (terminal observations: the host routes such calls to gpd_rollout_kernel -- a conditional
                        // store in this loop body would make the wait counts conservative again)
    RollOut<NT_OBS> ro(obs12, reward, terminated, truncated, T, goff, eoff4, L.env, sh_rows + tid * 12, lsrc);
    float irpy[3] = {0.0f, 0.0f, 0.0f};
    if (C.auto_reset) quat_to_rpy(ip[3], ip[4], ip[5], ip[6], irpy[0], irpy[1], irpy[2]);
    auto do_step = [&](const int t, const float4 act) {
        StepOut out;
        env_step<PID, EXT, MULTI, AW, ACT, S1>(Q, C, flags, D, L, act, tgx, tgy, tgz, true, ipose, ip[0], ip[1], ip[2], ip[3],
                                               ip[4], ip[5], ip[6], sh_pos, sh_red, c, out, irpy);
        ro.emit(out, t > 0);                                          // (see RollOut: pipelined bursts, unconditional stores)
        if constexpr (RING) {
            const size_t slot = static_cast<size_t>(N) * AW;
            float* r0 = S.act_ring + static_cast<size_t>(ring_q) * slot + static_cast<size_t>(L.n) * AW;
            float* r1 = r0 + static_cast<size_t>(S.hist_len) * slot;
            if (AW == 4) { *reinterpret_cast<float4*>(r0) = act; *reinterpret_cast<float4*>(r1) = act; }
            else { r0[0] = act.x; r1[0] = act.x; if (AW == 3) { r0[1] = act.y; r0[2] = act.z; r1[1] = act.y; r1[2] = act.z; } }
            ring_q = ring_q + 1 == S.hist_len ? 0 : ring_q + 1;
        }
    };
    // Action rows, three steps per loop iteration: the rows of the NEXT iteration (b0..b2) are requested at the top of
    // this one and claimed at its end with an explicit vmcnt(18) -- "everything but the youngest 18 operations", i.e.
    // but the 3 x 6 stores of this iteration's steps, has completed.  The rows had three steps of arithmetic to arrive,
    // the wait never touches a store younger than three steps, and no load is in flight across the loop's back edge
    // (where the compiler's wait-count bookkeeping would otherwise fall back to a wait for nearly every store).
    if (!PID) {
        float4 a0 = fetch(0), a1 = fetch(1), a2 = fetch(2);
        asm volatile("" :: "v"(a0.x), "v"(a0.y), "v"(a0.z), "v"(a0.w), "v"(a1.x), "v"(a1.y), "v"(a1.z), "v"(a1.w), "v"(a2.x),
                           "v"(a2.y), "v"(a2.z), "v"(a2.w) : "memory");
        __builtin_amdgcn_s_waitcnt(0x0F70);
        for (int t = 0; t < K; t += 3) {
            const float4 b0 = fetch(t + 3), b1 = fetch(t + 4), b2 = fetch(t + 5);
            do_step(t, a0);
            if (t + 1 >= K) break;
            do_step(t + 1, a1);
            if (t + 2 >= K) break;
            do_step(t + 2, a2);
            asm volatile("" :: "v"(b0.x), "v"(b0.y), "v"(b0.z), "v"(b0.w), "v"(b1.x), "v"(b1.y), "v"(b1.z), "v"(b1.w),
                               "v"(b2.x), "v"(b2.y), "v"(b2.z), "v"(b2.w) : "memory");
            a0 = b0; a1 = b1; a2 = b2;
        }
    } else {
        // DSLPID action types: the step body is ~2x longer (a row arrives within one step) and three copies of it would
        // not sit well in the instruction cache -- one step per iteration, the next row claimed with an exact vmcnt(6)
        float4 a = fetch(0);
        asm volatile("" :: "v"(a.x), "v"(a.y), "v"(a.z), "v"(a.w) : "memory");
        __builtin_amdgcn_s_waitcnt(0x0F70);
        for (int t = 0; t < K; ++t) {
            const float4 b = fetch(t + 1);
            do_step(t, a);
            asm volatile("" :: "v"(b.x), "v"(b.y), "v"(b.z), "v"(b.w) : "memory");
            a = b;
        }
    }
    ro.flush();                                                      // the last step's bursts
    if (L.active) store_carry<PID>(S, L, c);
    if constexpr (RING) { if (L.active && L.d == 0) S.ring_pos[L.env] = ring_q; }
}
