// rollout_kernel_body.inc -- the body of gpd_rollout_kernel and gpd_rollout_plant_kernel (step_rollout.hip), included INSIDE both __global__ functions.
// A textual body rather than a __device__ function on purpose: the kernels that existed before the plant path must compile to the same
// assembly, and a body called through a function (even always inlined, its LDS arrays declared in the kernels) does not -- the kernel
// argument loads lose their no-clobber annotation and the register allocation moves.  The including kernel defines PLANT (constexpr
// bool) and `plant` (the table, nullptr without one); with PLANT false, plant_of<false> is the argument struct itself.
{
    const int D = MULTI ? C.drones_per_env : 1;
    const int tid = threadIdx.x;
    const uint32_t N = static_cast<uint32_t>(C.num_envs) * static_cast<uint32_t>(D);
    const int lanes = MULTI ? (kBlock / D) * D : kBlock;             // drones per workgroup
    const uint32_t block_base = blockIdx.x * static_cast<uint32_t>(lanes);
    const uint32_t left = N - block_base;                            // > 0 by construction of the grid
    const int lanes_valid = left < static_cast<uint32_t>(lanes) ? static_cast<int>(left) : lanes;
    const int envs_block = lanes / D;
    const uint32_t env_base = blockIdx.x * static_cast<uint32_t>(envs_block);
    const int envs_valid = lanes_valid / D;
    const int K = T.num_steps;
    const uint32_t flags = EXT ? C.physics_flags : 0u;
    // multi-drone aviaries that fit D aligned lanes of a wave exchange wave-locally: no barrier inside a step
    const bool shfl = MULTI && D <= 64 && (D & (D - 1)) == 0;
    const bool use_flags = !MULTI || shfl;                           // hand-over protocol: LDS flags, or one barrier per step
    // workgroup barriers inside one env step (env_step): the store wave has to take part in each of them
    const int step_barriers = (MULTI && !shfl) ? (((flags & GPD_PHYS_DW) ? 2 * C.substeps : 0) + (C.task != GPD_TASK_NONE ? 2 : 0)) : 0;

    // Output ring: slot = step & (ring-1).  Single-drone aviaries hand over through flags (no barrier: a compute
    // wave never waits for its siblings, and only waits for the store wave when it is ring-1 steps ahead);
    // multi-drone aviaries already synchronise the workgroup inside every step (downwash snapshot, aviary
    // reductions) and keep the simpler two-slot, one-more-barrier-per-step hand-off.
    extern __shared__ __attribute__((aligned(16))) char sh_ring[];
    const int ring = use_flags ? T.ring : 2;
    auto slot_obs = [&](int b) { return reinterpret_cast<float*>(sh_ring + b * kSlotBytes); };
    auto slot_rew = [&](int b) { return reinterpret_cast<float*>(sh_ring + b * kSlotBytes + kBlock * 48); };
    auto slot_term = [&](int b) { return reinterpret_cast<uint8_t*>(sh_ring + b * kSlotBytes + kBlock * 52); };
    auto slot_trunc = [&](int b) { return reinterpret_cast<uint8_t*>(sh_ring + b * kSlotBytes + kBlock * 53); };
    __shared__ __attribute__((aligned(16))) int sh_prog[4];          // steps written, per compute wave
    __shared__ int sh_drained;                                       // steps copied to HBM by the store wave
    __shared__ __attribute__((aligned(16))) float sh_pos[MULTI ? 4 * kBlock : 4];
    __shared__ __attribute__((aligned(16))) float sh_red[MULTI ? 4 * kBlock : 4];
    if (use_flags) {
        if (tid < 4) sh_prog[tid] = 0;
        if (tid == 4) sh_drained = 0;
        wg_barrier();                                                // the only barrier of a flag-synchronised rollout
    }

    if (tid >= kBlock) {
        // ======================= store wave ===========================================================
        const int m = tid - kBlock;
        const bool full = lanes_valid == kBlock && envs_valid == kBlock &&
                          ((reinterpret_cast<uintptr_t>(terminated) | reinterpret_cast<uintptr_t>(truncated) |
                            static_cast<uintptr_t>(T.env_stride)) & 3) == 0;
        const uint32_t lane16 = static_cast<uint32_t>(m) * 16u;
        auto drain = [&](int step) {                                 // LDS slot of `step` -> HBM
            const int b = step & (ring - 1);
            char* og = reinterpret_cast<char*>(obs12 + step * T.obs_stride + static_cast<int64_t>(block_base) * 12);
            const char* ol = reinterpret_cast<const char*>(slot_obs(b));
            float* rg = reward + step * T.env_stride + env_base;
            uint8_t* tg = terminated + step * T.env_stride + env_base;
            uint8_t* ug = truncated + step * T.env_stride + env_base;
            if (full) {
                // a whole workgroup of single-drone aviaries: 12 + 1 unconditional 1 KiB bursts and two 256 B ones,
                // <uniform base> + <lane offset> + <immediate> addressing
                float4 v[12];
#pragma unroll
                for (int j = 0; j < 12; ++j) v[j] = *reinterpret_cast<const float4*>(ol + lane16 + j * 1024);
                const float4 rv = *reinterpret_cast<const float4*>(reinterpret_cast<const char*>(slot_rew(b)) + lane16);
                const uint32_t tv = reinterpret_cast<const uint32_t*>(slot_term(b))[m];
                const uint32_t uv = reinterpret_cast<const uint32_t*>(slot_trunc(b))[m];
#pragma unroll
                for (int j = 0; j < 12; ++j) {                       // (write-once streams: non-temporal)
                    f4v w = {v[j].x, v[j].y, v[j].z, v[j].w};
                    __builtin_nontemporal_store(w, reinterpret_cast<f4v*>(og + lane16 + j * 1024));
                }
                f4u w = {rv.x, rv.y, rv.z, rv.w};
                *reinterpret_cast<f4u*>(reinterpret_cast<char*>(rg) + lane16) = w;
                reinterpret_cast<uint32_t*>(tg)[m] = tv;
                reinterpret_cast<uint32_t*>(ug)[m] = uv;
                return;
            }
            const int chunks = lanes_valid * 3;                      // 16-byte chunks; chunk of lane m: j*64 + m
            float4 v[12];
#pragma unroll
            for (int j = 0; j < 12; ++j) v[j] = *reinterpret_cast<const float4*>(ol + lane16 + j * 1024);
#pragma unroll
            for (int j = 0; j < 12; ++j) {
                if (j * kStoreLanes + m < chunks) {
                    f4v w = {v[j].x, v[j].y, v[j].z, v[j].w};
                    __builtin_nontemporal_store(w, reinterpret_cast<f4v*>(og + lane16 + j * 1024));
                }
            }
            for (int e = m; e < envs_valid; e += kStoreLanes) {
                rg[e] = slot_rew(b)[e];
                tg[e] = slot_term(b)[e];
                ug[e] = slot_trunc(b)[e];
            }
        };
        __builtin_amdgcn_s_setprio(0);                               // fills the issue gaps of the compute wave it shares a SIMD with
        if (use_flags) {
            for (int t = 0; t < K; ++t) {
                for (;;) {                                           // until all four compute waves have written step t
                    const i4v pr = lds_peek4(sh_prog);
                    const int lo = min(min(pr.x, pr.y), min(pr.z, pr.w));
                    if (__builtin_amdgcn_readfirstlane(lo) > t) break;
                    __builtin_amdgcn_s_sleep(1);
                }
                drain(t);
                __builtin_amdgcn_s_waitcnt(0xC07F);                  // the slot has been read (lgkmcnt(0)) ...
                lds_poke(&sh_drained, t + 1);                        // ... and may be overwritten
            }
            return;
        }
        for (int t = 0; t < K; ++t) {
            for (int i = 0; i < step_barriers; ++i) wg_barrier();    // (the compute waves' env_step barriers)
            if (t > 0) drain(t - 1);                                 // overlaps the compute waves' step t
            wg_barrier();                                            // end of step t
        }
        drain(K - 1);
        return;
    }

    // ======================= compute waves ================================================================
    __builtin_amdgcn_s_setprio(2);
    Lane L;
    L.tid = tid;
    L.active = tid < lanes_valid;
    L.n = L.active ? block_base + tid : 0u;
    L.le = MULTI ? (tid < lanes ? tid / D : 0) : tid;
    L.d = MULTI ? (L.active ? tid - L.le * D : 0) : 0;
    L.env = MULTI ? (L.active ? env_base + L.le : 0u) : L.n;
    L.shfl = shfl;
    L.base = MULTI ? L.le * D : tid;

    Carry c;
    float tgx, tgy, tgz, ip[7];
    // Action rows are prefetched TWO steps ahead into three rotating register sets (a0, a1, a2): with the store
    // wave's bursts ahead of it in the CU's memory pipeline a row takes > 1 us to arrive, longer than one step.
    // The loop is unrolled by three so that the rotation needs no register copies (a copy of a set whose load is
    // still in flight would have to wait for it).  Past the last step the loads re-read the last block.
    auto fetch = [&](int step) { return load_action<AW>(action + (step < K ? step : K - 1) * T.action_stride, L.n); };
    // the rollout keeps its reset pose in registers: no dependent global load inside the step loop
    const float* ipose = reinterpret_cast<const float*>(reinterpret_cast<const char*>(init_pose) +
                                                        (C.init_per_env ? L.n * 28u : static_cast<uint32_t>(L.d) * 28u));
    load_carry<PID, EXT>(S, C, flags, L, target_pos, C.auto_reset ? ipose : S.kin, c, tgx, tgy, tgz, ip);
    // Everything requested above has to have arrived before the step loop starts (the empty asm makes the values
    // live here; the explicit wait lets the compiler's wait-count bookkeeping start the loop with nothing pending,
    // otherwise it would re-wait, conservatively, inside every iteration).
    asm volatile("" :: "v"(c.k.px), "v"(c.k.py), "v"(c.k.pz), "v"(c.k.qx), "v"(c.k.qy), "v"(c.k.qz), "v"(c.k.qw), "v"(c.k.vx),
                       "v"(c.k.vy), "v"(c.k.vz), "v"(c.k.wx), "v"(c.k.wy), "v"(c.k.wz), "v"(tgx), "v"(tgy), "v"(tgz), "v"(c.counter), "v"(ip[0]), "v"(ip[1]), "v"(ip[2]),
                       "v"(ip[3]), "v"(ip[4]), "v"(ip[5]), "v"(ip[6]) : "memory");
    __builtin_amdgcn_s_waitcnt(0x0F70);                              // vmcnt(0), expcnt/lgkmcnt untouched
    c.roll = c.pitch = c.yaw = 0.0f;
    if (PID) quat_to_rpy(c.k.qx, c.k.qy, c.k.qz, c.k.qw, c.roll, c.pitch, c.yaw);
    plant_t<PLANT> Q = plant_of<PLANT>(P, plant, S.ld, L.n * 4u);     // (PLANT: the drone's row, in registers for all K steps)

    float* const tobs_t = term_obs12;
    int drained_seen = 0;                                            // last value of sh_drained this wave has read
    auto do_step = [&](const int t, const float4 act) {
        StepOut out;
        env_step<PID, EXT, MULTI, AW, ACT, S1>(Q, C, flags, D, L, act, tgx, tgy, tgz, true, ipose, ip[0], ip[1], ip[2], ip[3], ip[4],
                                               ip[5], ip[6], sh_pos, sh_red, c, out);
        const int b = t & (ring - 1);
        if (use_flags && t - ring + 1 > drained_seen) {              // slot b may still hold step t-ring: has it been drained?
            // (the flag is re-read only when the last value seen does not already clear this step: the store wave
            // normally runs one step behind, so one read clears the next ring-1 steps)
            while ((drained_seen = __builtin_amdgcn_readfirstlane(lds_peek(&sh_drained))) < t - ring + 1)
                __builtin_amdgcn_s_sleep(1);
        }
        float4* ol = reinterpret_cast<float4*>(slot_obs(b) + tid * 12);
        ol[0] = make_float4(out.o[0], out.o[1], out.o[2], out.o[3]);
        ol[1] = make_float4(out.o[4], out.o[5], out.o[6], out.o[7]);
        ol[2] = make_float4(out.o[8], out.o[9], out.o[10], out.o[11]);
        if (!MULTI || (L.active && L.d == 0)) {                      // (single-drone aviaries: every lane owns a slot)
            slot_rew(b)[L.le] = out.rew;
            slot_term(b)[L.le] = out.term ? 1 : 0;
            slot_trunc(b)[L.le] = out.trunc ? 1 : 0;
        }
        if (out.reset && tobs_t && L.active) {
            // Terminal observation of an aviary that ended (rare).  Issued through inline asm on purpose: the
            // compiler's wait-count pass does not see these stores, so they cannot make its waits for the
            // action prefetch conservative (vmcnt(0) in every iteration); stores the pass does not know about can
            // only make a counter-based wait longer, never too short (vmcnt is in-order).
            float* row = reinterpret_cast<float*>(reinterpret_cast<char*>(tobs_t + t * T.obs_stride) + L.n * 48u);
            f4v q0 = {out.to[0], out.to[1], out.to[2], out.to[3]}, q1 = {out.to[4], out.to[5], out.to[6], out.to[7]},
                q2 = {out.to[8], out.to[9], out.to[10], out.to[11]};
            asm volatile("global_store_dwordx4 %0, %1, off\n\tglobal_store_dwordx4 %0, %2, off offset:16\n\t"
                         "global_store_dwordx4 %0, %3, off offset:32" :: "v"(row), "v"(q0), "v"(q1), "v"(q2) : "memory");
        }
        if (!use_flags) wg_barrier();                                // end of step t
        else lds_poke(&sh_prog[tid >> 6], t + 1);                    // this wave's rows of step t are in the slot
    };
    // (a0 and a1 are requested AFTER the wait above, so that the loop is entered in the state every iteration
    // leaves behind -- two rows in flight, a0 the older -- and the compiler's wait counts stay exact)
    if (!PID) {
        float4 a0 = fetch(0), a1, a2;
        __builtin_amdgcn_sched_barrier(0);                           // (a0 must be the older of the two)
        a1 = fetch(1);
        __builtin_amdgcn_sched_barrier(0);
        for (int t = 0; t < K; t += 3) {
            a2 = fetch(t + 2);
            do_step(t, a0);
            if (t + 1 >= K) break;
            a0 = fetch(t + 3);
            do_step(t + 1, a1);
            if (t + 2 >= K) break;
            a1 = fetch(t + 4);
            do_step(t + 2, a2);
        }
    } else {
        // The DSLPID step body is ~2x longer (the row has time to arrive within one step) and three copies of it
        // would not sit well in the instruction cache: one step of look-ahead, one copy of the body.
        float4 act = fetch(0);
        for (int t = 0; t < K; ++t) {
            const float4 act_next = fetch(t + 1);
            do_step(t, act);
            act = act_next;
        }
    }
    if (L.active) store_carry<PID>(S, L, c);
}
