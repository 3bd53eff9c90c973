// step_kernel_body.inc -- the body of gpd_step_kernel and gpd_step_plant_kernel (step_rollout.hip), included INSIDE both __global__ functions.
// A textual body rather than a __device__ function on purpose: the kernels that existed before the plant path must compile to the same
// assembly, and a body called through a function (even always inlined, its LDS arrays declared in the kernels) does not -- the kernel
// argument loads lose their no-clobber annotation and the register allocation moves.  The including kernel defines PLANT (constexpr
// bool) and `plant` (the table, nullptr without one); with PLANT false, plant_of<false> is the argument struct itself.
{
    // (built member by member: a copy of the argument struct with three members overwritten stays an 80-byte alloca in the EXT variants --
    // the `flag ? S.last_rpm : S.kin` selects become loads from a selected ADDRESS inside it -- i.e. scratch memory, and a launch that
    // needs scratch costs 1.6 us more: hover65536_ext 5.07 -> 6.65 us per step, gpurun_out/bench_r05.log of the first round-5 build)
    const GpdState S{hot_kin, S_.last_rpm, S_.pid, hot_counter, static_cast<int64_t>(hot_ld), S_.dw_force, S_.act_ring, S_.ring_pos, S_.hist_len, 0, S_.bad};
    const GpdStepCfg C{hot_num_envs, C_.drones_per_env, C_.act_type, C_.substeps, C_.physics_flags, C_.pyb_dt, C_.ctrl_dt, C_.inv_ctrl_dt,
                       hot_lanes_per_wave, C_.task, C_.xy_bound, C_.z_bound, C_.tilt_bound, C_.term_dist, C_.trunc_counter, hot_target_per_env,
                       C_.init_per_env, C_.auto_reset};
    const int D = MULTI ? (DC ? DC : C.drones_per_env) : 1;
    const int tid = threadIdx.x;
    const uint32_t N = static_cast<uint32_t>(C.num_envs) * static_cast<uint32_t>(D);
    // MULTI: whole aviaries per workgroup, one lane per drone.  Single-drone aviaries: LW = lanes_per_wave
    // (16/32/64) active lanes per 64-wide wavefront (tuning knob, see GpdStepCfg).
    const int LW = MULTI ? 64 : C.lanes_per_wave;
    const int lanes = MULTI ? (kBlock / D) * D : (kBlock / 64) * LW;
    const uint32_t n_raw = MULTI ? blockIdx.x * lanes + tid : (blockIdx.x * (kBlock / 64) + (tid >> 6)) * LW + (tid & 63);
    Lane L;
    L.tid = tid;
    L.active = (MULTI ? (tid < lanes) : ((tid & 63) < LW)) && (n_raw < N);
    L.n = L.active ? n_raw : 0u;
    L.le = MULTI ? (tid < lanes ? tid / D : 0) : tid;
    L.d = MULTI ? (L.active ? tid - L.le * D : 0) : 0;
    L.env = MULTI ? (L.active ? blockIdx.x * (lanes / D) + L.le : 0u) : L.n;
    L.shfl = MULTI && D <= 64 && (D & (D - 1)) == 0;
    L.base = MULTI ? L.le * D : tid;

    __shared__ __attribute__((aligned(16))) float sh_pos[MULTI ? 4 * kBlock : 4];   // downwash: positions of the env's drones
    __shared__ __attribute__((aligned(16))) float sh_red[MULTI ? 4 * kBlock : 4];   // reward | distance | out-of-bounds per drone
    __shared__ __attribute__((aligned(16))) float sh_rows[kBlock * 12];   // obs rows, for the coalesced store of large batches

    const uint32_t flags = EXT ? (FL >= 0 ? (static_cast<uint32_t>(FL) | (HI ? C.physics_flags & ~7u : 0u)) : C.physics_flags) : 0u;
    Carry c;
    float tgx, tgy, tgz;
    const float4 act = load_action<AW>(action, L.n);
    // action history: the slot this aviary's action goes to (read with the other loads, from a readable dummy when there is
    // no ring: the load section stays branch-free)
    int ring_q = hot_slot[L.env];
    if (S.act_ring) { GPD_DBG(ring_q >= 0 && ring_q < S.hist_len, GPD_DBG_RING_POS, ring_q); ring_q = GPD_DBG_CLAMP(ring_q, 0, S.hist_len - 1); }
    // a single step reads its reset pose only if it resets (in env_step)
    const float* ipose = reinterpret_cast<const float*>(reinterpret_cast<const char*>(init_pose) +
                                                        (C.init_per_env ? L.n * 28u : static_cast<uint32_t>(L.d) * 28u));
    load_carry<PID, EXT, false>(S, C, flags, L, target_pos, nullptr, c, tgx, tgy, tgz, nullptr);
    // An aviary that spans several waves of the workgroup (D not a power of two <= 64): its lane 0 publishes ring_pos + 1 at
    // the end of this kernel, and with no task and no downwash nothing else synchronises the waves -- every wave must have
    // READ ring_pos before any of them gets there (the barrier also waits for the loads above: vmcnt(0))
    if (MULTI && !L.shfl && S.act_ring) __syncthreads();
    c.roll = c.pitch = c.yaw = 0.0f;
    if (PID) quat_to_rpy(c.k.qx, c.k.qy, c.k.qz, c.k.qw, c.roll, c.pitch, c.yaw);
    plant_t<PLANT> Q = plant_of<PLANT>(P, plant, S.ld, L.n * 4u);     // (PLANT: the drone's row; otherwise P itself)

    StepOut out;
    env_step<PID, EXT, MULTI, AW, ACT, S1>(Q, C, flags, D, L, act, tgx, tgy, tgz, false, ipose, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f,
                                           0.0f, 0.0f, sh_pos, sh_red, c, out);
    // Observation rows.  A lane's row is 48 bytes, so a wave's direct stores are 48-byte-strided pieces of cache
    // lines; in the bandwidth-bound regime (large batches) the wave transposes its 64 rows through LDS and
    // stores three fully coalesced 1 KiB bursts instead (the rows of a wave are contiguous in memory); narrower waves
    // (lanes_per_wave < 64, a tuning knob) store directly.
    // (round 1 kept direct 48-byte row stores below 2^18 drones; a round-2 A/B on one box has the transposed bursts ahead at
    // every size: 4.74 -> 4.38 us per step at N = 65 536, -8..10 % with DSLPID / 8 sub-steps / 8-drone aviaries, equal at 4 096)
    const bool big = C.lanes_per_wave == 64;
    if (big) {
        float4* mine = reinterpret_cast<float4*>(sh_rows + tid * 12);
        mine[0] = make_float4(out.o[0], out.o[1], out.o[2], out.o[3]);
        mine[1] = make_float4(out.o[4], out.o[5], out.o[6], out.o[7]);
        mine[2] = make_float4(out.o[8], out.o[9], out.o[10], out.o[11]);
        const int wave0 = tid & ~63;                                  // first lane of this wave
        const uint32_t n0 = n_raw - static_cast<uint32_t>(tid & 63);  // first drone of this wave
        if (n0 < N) {
            // valid rows of this wave: its lanes that own a drone (whole aviaries per workgroup: `lanes` may be < 256)
            uint32_t rows = static_cast<uint32_t>(lanes - wave0 < 64 ? (lanes - wave0 > 0 ? lanes - wave0 : 0) : 64);
            if (N - n0 < rows) rows = N - n0;
            const char* src = reinterpret_cast<const char*>(sh_rows + wave0 * 12);
            char* dst = reinterpret_cast<char*>(obs12) + static_cast<size_t>(n0) * 48u;
            const uint32_t off = static_cast<uint32_t>(tid & 63) * 16u;
            __builtin_amdgcn_wave_barrier();                          // same wave: the LDS executes its instructions in order
            if (rows == 64u) {
                // a full wave (every wave but a ragged batch's last): the three reads in one run, one wait, three unconditional stores --
                // the masked form below reads, waits and stores three times over (three LDS round trips on the tail of the kernel)
                const float4 v0 = *reinterpret_cast<const float4*>(src + off), v1 = *reinterpret_cast<const float4*>(src + off + 1024),
                             v2 = *reinterpret_cast<const float4*>(src + off + 2048);
                __builtin_nontemporal_store(f4v{v0.x, v0.y, v0.z, v0.w}, reinterpret_cast<f4v*>(dst + off));
                __builtin_nontemporal_store(f4v{v1.x, v1.y, v1.z, v1.w}, reinterpret_cast<f4v*>(dst + off + 1024));
                __builtin_nontemporal_store(f4v{v2.x, v2.y, v2.z, v2.w}, reinterpret_cast<f4v*>(dst + off + 2048));
            } else {
#pragma unroll
                for (int j = 0; j < 3; ++j) {
                    const float4 v = *reinterpret_cast<const float4*>(src + off + j * 1024);
                    if (off + j * 1024 < rows * 48u) {                // streamed out, not read again by this path: non-temporal
                        f4v w = {v.x, v.y, v.z, v.w};
                        __builtin_nontemporal_store(w, reinterpret_cast<f4v*>(dst + off + j * 1024));
                    }
                }
            }
        }
        if (!L.active) return;
    } else {
        if (!L.active) return;
        store_obs12(obs12, L.n, out.o[0], out.o[1], out.o[2], out.o[3], out.o[4], out.o[5], out.o[6], out.o[7], out.o[8],
                    out.o[9], out.o[10], out.o[11]);
    }
    if (L.d == 0) {
        // (written once, read by another kernel: non-temporal like the observation bursts -- 4.38 -> 4.30 us per step, A/B)
        __builtin_nontemporal_store(out.rew, &reward[L.env]);
        __builtin_nontemporal_store(static_cast<uint8_t>(out.term ? 1 : 0), &terminated[L.env]);
        __builtin_nontemporal_store(static_cast<uint8_t>(out.trunc ? 1 : 0), &truncated[L.env]);
    }
    if (S.act_ring) {
        // push the raw action into the double ring (slots q and q + H: the H most recent actions stay H consecutive slots);
        // a slot is a contiguous [N][A] block, so this is the coalesced mirror image of the action load
        const size_t slot = static_cast<size_t>(N) * AW, at = static_cast<size_t>(ring_q) * slot + static_cast<size_t>(L.n) * AW;
        float* r0 = S.act_ring + at;
        float* r1 = r0 + static_cast<size_t>(S.hist_len) * slot;
        if (AW == 4) {
            *reinterpret_cast<float4*>(r0) = act;
            *reinterpret_cast<float4*>(r1) = act;
        } else {
            r0[0] = act.x; r1[0] = act.x;
            if (AW == 3) { r0[1] = act.y; r0[2] = act.z; r1[1] = act.y; r1[2] = act.z; }
        }
        if (L.d == 0) S.ring_pos[L.env] = ring_q + 1 == S.hist_len ? 0 : ring_q + 1;
    }
    if (out.reset && term_obs12)
        store_obs12(term_obs12, L.n, out.to[0], out.to[1], out.to[2], out.to[3], out.to[4], out.to[5], out.to[6], out.to[7],
                    out.to[8], out.to[9], out.to[10], out.to[11]);
    // the state block is streamed out non-temporally at every size: nothing of this launch reads it again, and the next launch's loads
    // miss the XCD-private L2 either way (round 5 A/B, profiles/r05_ab_step_kernel_round2.log: 3.95 -> 3.93 us per step at 65 536 drones,
    // 2.91 -> 2.87 at 4 096, equal at 4 194 304; rounds 1-4 kept ordinary stores up to 2^22 drones)
    store_carry<PID, true>(S, L, c);
    signal_done(done_flag, done_seq, L.n == 0u);         // (gpd_step_sync on a one-wave launch; NULL otherwise -- gpd_common.inc)
}
