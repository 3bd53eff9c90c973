// mrac.hip -- the reference's model-reference adaptive controller (control/MRAC.py) on the device: the batched computeControl
// (gpd_mrac), its reset (gpd_mrac_reset) and the rollout with the controller IN the loop (gpd_rollout_mrac).  DESIGN.md section 3.11.
//
// One lane per controller.  The 76 floats of controller state (Kx 12x4 | Kr 4x4 | Xm 12) and every constant matrix of GpdMrac are
// indexed with compile-time indices only (fully unrolled loops): the state lives in VGPRs, the constants are wave-uniform.
// `mrac_rt` + `mrac_call` are the ONE statement of the controller's arithmetic, shared by both kernels: fp32, contraction off, every
// fused multiply-add an explicit fmaf() in one fixed order, so that gpd_step + gpd_mrac and gpd_rollout_mrac agree bit for bit.
#include "gpd_common.inc"

namespace {

struct MracState {
    float Kx[48];      // [12][4]
    float Kr[16];      // [4][4]
    float Xm[12];
};

__device__ __forceinline__ void mrac_load(const float* __restrict__ st, int64_t ld, uint32_t off4, MracState& m) {
#pragma unroll
    for (int i = 0; i < 48; ++i) m.Kx[i] = ld_row(st, ld, i, off4);
#pragma unroll
    for (int i = 0; i < 16; ++i) m.Kr[i] = ld_row(st, ld, 48 + i, off4);
#pragma unroll
    for (int i = 0; i < 12; ++i) m.Xm[i] = ld_row(st, ld, 64 + i, off4);
}

__device__ __forceinline__ void mrac_store(float* __restrict__ st, int64_t ld, uint32_t off4, const MracState& m) {
#pragma unroll
    for (int i = 0; i < 48; ++i) st_row(st, ld, i, off4, m.Kx[i]);
#pragma unroll
    for (int i = 0; i < 16; ++i) st_row(st, ld, 48 + i, off4, m.Kr[i]);
#pragma unroll
    for (int i = 0; i < 12; ++i) st_row(st, ld, 64 + i, off4, m.Xm[i]);
}

// The design's constants (the first kHot floats of GpdMrac: everything but Kx0 / Kr0) are ~180 values, every one of them read once
// per control step: far more than the scalar registers hold next to GpdParams.  Left in the kernel-argument segment the compiler
// loads them all ahead of the step loop and spills them to VGPR lanes (170-380 spills, one v_readlane per use, scratch memory in
// one instantiation).  So every wave copies them ONCE into an LDS block of its own (a wave's LDS operations execute in order: no
// barrier) and a control step reads them back as 16-byte broadcasts -- 32 ds_read_b128 per step (44 with a target row per step),
// in-order counted waits.  The block's pointer is made opaque once per step, otherwise the reads are loop-invariant and hoisted
// into ~180 VGPRs.
constexpr int kHot = static_cast<int>(offsetof(GpdMrac, Kx0) / sizeof(float));     // 176 floats
static_assert(kHot % 4 == 0 && offsetof(GpdMrac, PB) == 0, "GpdMrac: the hot part is read as float4 rows");
typedef const __attribute__((address_space(3))) f4v* lds4;
constexpr int kPB = 0, kGain = static_cast<int>(offsetof(GpdMrac, Kr_ref_gain) / 16), kAm = static_cast<int>(offsetof(GpdMrac, Am_lo) / 16),
              kGrav = static_cast<int>(offsetof(GpdMrac, A_grav) / 16), kBd = static_cast<int>(offsetof(GpdMrac, B_diag) / 16),
              kMix = static_cast<int>(offsetof(GpdMrac, mixer) / 16), kGam = static_cast<int>(offsetof(GpdMrac, gamma_x) / 16),
              kPwm = static_cast<int>(offsetof(GpdMrac, pwm2rpm_scale) / 16), kMax = static_cast<int>(offsetof(GpdMrac, max_pwm) / 16);

__device__ __forceinline__ void mrac_stage(const GpdMrac& M, float* __restrict__ sh) {     // sh: this wave's kHot floats, 16-byte aligned
    f4v* d = reinterpret_cast<f4v*>(sh);
#pragma unroll
    for (int i = 0; i < 12; ++i) {
        d[kPB + i] = f4v{M.PB[4 * i], M.PB[4 * i + 1], M.PB[4 * i + 2], M.PB[4 * i + 3]};
        d[kGain + i] = f4v{M.Kr_ref_gain[4 * i], M.Kr_ref_gain[4 * i + 1], M.Kr_ref_gain[4 * i + 2], M.Kr_ref_gain[4 * i + 3]};
        d[kAm + i] = f4v{M.Am_lo[4 * i], M.Am_lo[4 * i + 1], M.Am_lo[4 * i + 2], M.Am_lo[4 * i + 3]};
    }
    d[kGrav] = f4v{M.A_grav[0], M.A_grav[1], M.A_grav[2], M.A_grav[3]};
    d[kBd] = f4v{M.B_diag[0], M.B_diag[1], M.B_diag[2], M.B_diag[3]};
#pragma unroll
    for (int i = 0; i < 3; ++i) d[kMix + i] = f4v{M.mixer[4 * i], M.mixer[4 * i + 1], M.mixer[4 * i + 2], M.mixer[4 * i + 3]};
    d[kGam] = f4v{M.gamma_x, M.gamma_r, M.inv_4kf, M.max_torque};
    d[kPwm] = f4v{M.pwm2rpm_scale, M.inv_pwm2rpm_scale, M.pwm2rpm_const, M.min_pwm};
    d[kMax] = f4v{M.max_pwm, 0.0f, 0.0f, 0.0f};
}

__device__ __forceinline__ lds4 mrac_consts(const float* sh) {
    lds4 p = (lds4)(sh);
    asm volatile("" : "+v"(p));          // (opaque: the reads below belong to THIS control step)
    return p;
}

// twelve floats against three float4 of constants: a0*x0, then fma by fma in index order (the one order both kernels share)
__device__ __forceinline__ float dot12(const f4v c0, const f4v c1, const f4v c2, const float x[12]) {
#pragma clang fp contract(off)
    float a = c0.x * x[0];
    a = fmaf(c0.y, x[1], a); a = fmaf(c0.z, x[2], a); a = fmaf(c0.w, x[3], a);
    a = fmaf(c1.x, x[4], a); a = fmaf(c1.y, x[5], a); a = fmaf(c1.z, x[6], a); a = fmaf(c1.w, x[7], a);
    a = fmaf(c2.x, x[8], a); a = fmaf(c2.y, x[9], a); a = fmaf(c2.z, x[10], a); a = fmaf(c2.w, x[11], a);
    return a;
}

// sin and cos of an Euler angle (|x| <= 2 pi: quat_to_rpy's range), branch-free: quadrant k = rint(2x/pi), r = x - k pi/2 in three
// exact-product steps (Cody-Waite), the single-precision minimax pair on [-pi/4, pi/4], quadrant fix-up by selects.  Absolute error
// <= 9e-8 on [-2 pi, 2 pi].  (OCML's sincosf carries its large-argument reduction as divergent blocks: six skipped branches per call
// of the controller, ~60 cycles each at one wave per SIMD.)
__device__ __forceinline__ void sincos_euler(const float x, float& sn, float& cs) {
#pragma clang fp contract(off)
    const float kf = rintf(x * 0.636619772f);
    const int q = static_cast<int>(kf);
    float r = fmaf(kf, -1.5703125f, x);
    r = fmaf(kf, -4.837512969970703125e-4f, r);
    r = fmaf(kf, -7.54978995489188216e-8f, r);
    const float z = r * r;
    const float ps = fmaf(fmaf(-1.9515295891e-4f, z, 8.3321608736e-3f), z, -1.6666654611e-1f);
    const float S = fmaf(ps * z, r, r);
    const float pc = fmaf(fmaf(2.443315711809948e-5f, z, -1.388731625493765e-3f), z, 4.166664568298827e-2f);
    const float C = fmaf(pc, z * z, fmaf(-0.5f, z, 1.0f));
    const bool swap = (q & 1) != 0;
    const float s0 = swap ? C : S, c0 = swap ? S : C;
    sn = (q & 2) ? -s0 : s0;
    cs = ((q + 1) & 2) ? -c0 : c0;
}

// rt = -Kr_ref_gain r (:127-128), r = target pos | rpy | vel | rpy rates.  A function of the target row alone: the rollout kernel
// evaluates it once per target row it reads (once per launch for a held target), the same operations as once per call.
__device__ __forceinline__ void mrac_rt(lds4 c, const float r[12], float rt[4]) {
#pragma clang fp contract(off)
#pragma unroll
    for (int j = 0; j < 4; ++j) rt[j] = -dot12(c[kGain + 3 * j], c[kGain + 3 * j + 1], c[kGain + 3 * j + 2], r);
}

// The rest of MRAC.computeControl (control/MRAC.py:109-155) for one controller, in the reference's order.
//   X[0..8]   pos | rpy | vel of the drone (rpy: quat_to_rpy of its quaternion, :120); wx, wy, wz: its WORLD angular velocity
//   rt        mrac_rt of the call's target row
//   c         the design's constants (mrac_consts)
__device__ __forceinline__ void mrac_call(lds4 c, const float dt, float X[12], const float wx, const float wy, const float wz,
                                          const float rt[4], MracState& m, int& counter, float rpm[4]) {
#pragma clang fp contract(off)
    // ---- body rates, :121: Rotation.from_euler('XYZ', rpy).inv().apply(w) -- intrinsic XYZ is R = Rx(roll) Ry(pitch) Rz(yaw), its
    // inverse applied to w is Rz(-yaw) Ry(-pitch) Rx(-roll) w: three plane rotations
    float sr, cr, sp, cp, sy, cy;
    sincos_euler(X[3], sr, cr);
    sincos_euler(X[4], sp, cp);
    sincos_euler(X[5], sy, cy);
    const float ay = fmaf(cr, wy, sr * wz), az = fmaf(cr, wz, -(sr * wy));              // Rx(-roll)
    const float bx = fmaf(cp, wx, -(sp * az)), bz = fmaf(cp, az, sp * wx);              // Ry(-pitch)
    X[9] = fmaf(cy, bx, sy * ay); X[10] = fmaf(cy, ay, -(sy * bx)); X[11] = bz;         // Rz(-yaw)
    // ---- the reference model starts where the drone is, :123-125
    const bool first = counter == 0;
#pragma unroll
    for (int i = 0; i < 12; ++i) m.Xm[i] = first ? X[i] : m.Xm[i];
    counter += 1;
    // ---- u = Kx^T X + Kr^T rt with the gains before this call's update, :131
    float u[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        float a = m.Kx[j] * X[0];
#pragma unroll
        for (int i = 1; i < 12; ++i) a = fmaf(m.Kx[4 * i + j], X[i], a);
#pragma unroll
        for (int k = 0; k < 4; ++k) a = fmaf(m.Kr[4 * k + j], rt[k], a);
        u[j] = a;
    }
    // ---- adaptation, :132-137: s = e^T (P Bm); Kx += -gamma_x X s dt; Kr += -gamma_r rt s dt
    const f4v gam = c[kGam];                     // gamma_x, gamma_r, inv_4kf, max_torque
    float s[4];
    {
        const f4v pb = c[kPB];
        const float e0 = X[0] - m.Xm[0];
        s[0] = e0 * pb.x; s[1] = e0 * pb.y; s[2] = e0 * pb.z; s[3] = e0 * pb.w;
    }
#pragma unroll
    for (int i = 1; i < 12; ++i) {
        const f4v pb = c[kPB + i];
        const float e = X[i] - m.Xm[i];
        s[0] = fmaf(e, pb.x, s[0]); s[1] = fmaf(e, pb.y, s[1]); s[2] = fmaf(e, pb.z, s[2]); s[3] = fmaf(e, pb.w, s[3]);
    }
    const float gx = -(gam.x * dt), gr = -(gam.y * dt);
    float sx[4], sk[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) { sx[j] = gx * s[j]; sk[j] = gr * s[j]; }
#pragma unroll
    for (int i = 0; i < 12; ++i) {
#pragma unroll
        for (int j = 0; j < 4; ++j) m.Kx[4 * i + j] = fmaf(X[i], sx[j], m.Kx[4 * i + j]);
    }
#pragma unroll
    for (int k = 0; k < 4; ++k) {
#pragma unroll
        for (int j = 0; j < 4; ++j) m.Kr[4 * k + j] = fmaf(rt[k], sk[j], m.Kr[4 * k + j]);
    }
    // ---- thrust and torques -> PWM -> RPM, :139-147
    const f4v pw = c[kPwm];                      // pwm2rpm_scale, its inverse, pwm2rpm_const, min_pwm
    const float max_pwm = c[kMax].x;
    const float thrust = fmaxf(0.0f, u[0]);
    const float t0 = clampf(u[1], -gam.w, gam.w), t1 = clampf(u[2], -gam.w, gam.w), t2 = clampf(u[3], -gam.w, gam.w);
    const float base_pwm = (fast_sqrt(thrust * gam.z) - pw.z) * pw.y;
    const f4v mx0 = c[kMix], mx1 = c[kMix + 1], mx2 = c[kMix + 2];
    const float mix[12] = {mx0.x, mx0.y, mx0.z, mx0.w, mx1.x, mx1.y, mx1.z, mx1.w, mx2.x, mx2.y, mx2.z, mx2.w};
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        const float pwm = clampf(fmaf(mix[3 * q + 2], t2, fmaf(mix[3 * q + 1], t1, fmaf(mix[3 * q], t0, base_pwm))), pw.w, max_pwm);
        rpm[q] = fmaf(pw.x, pwm, pw.z);
    }
    // ---- the reference model advances, :152-153: Xm += (Am Xm + Bm rt) dt.  Rows 0..5 of Am are [0 I], rows 6, 7 gravity's entries,
    // rows 8..11 dense; Bm is diagonal in its last four rows (include/gpd.h: the full product adds exact zeros to these sums)
    float xd[12];
    const f4v ag = c[kGrav], bd = c[kBd];
#pragma unroll
    for (int i = 0; i < 6; ++i) xd[i] = m.Xm[6 + i];
    xd[6] = fmaf(ag.y, m.Xm[4], ag.x * m.Xm[3]);
    xd[7] = fmaf(ag.w, m.Xm[4], ag.z * m.Xm[3]);
    const float bdk[4] = {bd.x, bd.y, bd.z, bd.w};
#pragma unroll
    for (int k = 0; k < 4; ++k) xd[8 + k] = fmaf(bdk[k], rt[k], dot12(c[kAm + 3 * k], c[kAm + 3 * k + 1], c[kAm + 3 * k + 2], m.Xm));
#pragma unroll
    for (int i = 0; i < 12; ++i) m.Xm[i] = fmaf(xd[i], dt, m.Xm[i]);
}

// ------------------------------------------------------------------------------------------------
// standalone batched MRAC.computeControl
// ------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(kBlock) void gpd_mrac_kernel(
    const GpdMrac M, float* __restrict__ mst, int32_t* __restrict__ counter, const int64_t ld, const float dt,
    const float* __restrict__ cur_pos, const float* __restrict__ cur_quat, const float* __restrict__ cur_vel,
    const float* __restrict__ cur_ang_vel, const float* __restrict__ target_pos, const float* __restrict__ target_rpy,
    const float* __restrict__ target_vel, const float* __restrict__ target_rpy_rates, float* __restrict__ rpm_out,
    float* __restrict__ pos_e_out, float* __restrict__ rpy_e_out, const int n_total) {
    __shared__ __attribute__((aligned(16))) float sh_m[(kBlock / 64) * kHot];
    const uint32_t n = blockIdx.x * static_cast<uint32_t>(kBlock) + threadIdx.x;
    if (n >= static_cast<uint32_t>(n_total)) return;
    float* const sh = sh_m + (threadIdx.x >> 6) * kHot;
    mrac_stage(M, sh);
    const uint32_t off4 = n * 4u, n3 = n * 3u;
    MracState m;
    mrac_load(mst, ld, off4, m);
    int ctr = counter[n];
    float X[12], r[12];
    X[0] = cur_pos[n3]; X[1] = cur_pos[n3 + 1]; X[2] = cur_pos[n3 + 2];
    const float4 q = reinterpret_cast<const float4*>(cur_quat)[n];
    X[6] = cur_vel[n3]; X[7] = cur_vel[n3 + 1]; X[8] = cur_vel[n3 + 2];
    const float wx = cur_ang_vel[n3], wy = cur_ang_vel[n3 + 1], wz = cur_ang_vel[n3 + 2];
    r[0] = target_pos[n3]; r[1] = target_pos[n3 + 1]; r[2] = target_pos[n3 + 2];
#pragma unroll
    for (int i = 3; i < 12; ++i) r[i] = 0.0f;
    if (target_rpy) { r[3] = target_rpy[n3]; r[4] = target_rpy[n3 + 1]; r[5] = target_rpy[n3 + 2]; }
    if (target_vel) { r[6] = target_vel[n3]; r[7] = target_vel[n3 + 1]; r[8] = target_vel[n3 + 2]; }
    if (target_rpy_rates) { r[9] = target_rpy_rates[n3]; r[10] = target_rpy_rates[n3 + 1]; r[11] = target_rpy_rates[n3 + 2]; }
    quat_to_rpy(q.x, q.y, q.z, q.w, X[3], X[4], X[5]);
    float rpm[4];
    float rt[4];
    const lds4 c = mrac_consts(sh);
    mrac_rt(c, r, rt);
    mrac_call(c, dt, X, wx, wy, wz, rt, m, ctr, rpm);
    mrac_store(mst, ld, off4, m);
    counter[n] = ctr;
    reinterpret_cast<float4*>(rpm_out)[n] = make_float4(rpm[0], rpm[1], rpm[2], rpm[3]);
    if (pos_e_out) { pos_e_out[n3] = r[0] - X[0]; pos_e_out[n3 + 1] = r[1] - X[1]; pos_e_out[n3 + 2] = r[2] - X[2]; }
    if (rpy_e_out) { rpy_e_out[n3] = r[3] - X[3]; rpy_e_out[n3 + 1] = r[4] - X[4]; rpy_e_out[n3 + 2] = r[5] - X[5]; }
}

// MRAC.reset (:106-107): the counter and nothing else -- the next call re-seeds Xm, the adapted gains survive
__global__ __launch_bounds__(kBlock) void gpd_mrac_reset_kernel(int32_t* __restrict__ counter, const uint8_t* __restrict__ mask,
                                                                const int n_total) {
    const uint32_t n = blockIdx.x * static_cast<uint32_t>(kBlock) + threadIdx.x;
    if (n >= static_cast<uint32_t>(n_total)) return;
    if (mask && !mask[n]) return;
    counter[n] = 0;
}

// ... and the extra: Kx0 | Kr0 of the design back into the state rows (64 wave-uniform floats by value: the library owns no memory)
struct Gains0 { float v[64]; };
__global__ __launch_bounds__(kBlock) void gpd_mrac_restore_kernel(float* __restrict__ mst, const int64_t ld, const Gains0 g,
                                                                  const uint8_t* __restrict__ mask, const int n_total) {
    const uint32_t n = blockIdx.x * static_cast<uint32_t>(kBlock) + threadIdx.x;
    if (n >= static_cast<uint32_t>(n_total)) return;
    if (mask && !mask[n]) return;
#pragma unroll
    for (int i = 0; i < 64; ++i) st_row(mst, ld, i, n * 4u, g.v[i]);
}

// ------------------------------------------------------------------------------------------------
// K control steps per launch, the controller in the loop (single-drone aviaries)
// ------------------------------------------------------------------------------------------------
struct Tgt { float4 a, b, c; };
__device__ __forceinline__ Tgt load_target(const float* __restrict__ rows, uint32_t n) {
    const float4* p = reinterpret_cast<const float4*>(reinterpret_cast<const char*>(rows) + n * 48u);
    return Tgt{p[0], p[1], p[2]};
}

template <bool EXT, bool PLANT>
__global__ __launch_bounds__(kBlock) void gpd_rollout_mrac_kernel(
    const GpdParams P, const GpdMrac M, float* __restrict__ kin, float* __restrict__ last_rpm, int32_t* __restrict__ step_counter,
    uint8_t* __restrict__ bad, const uint32_t ld32, const GpdStepCfg C, float* __restrict__ mst, int32_t* __restrict__ mcounter,
    const int64_t mld, const float* __restrict__ targets, const int64_t tstride, float* __restrict__ rpm_carry,
    const float* __restrict__ plant, float* __restrict__ obs12, const int64_t ostride, const int K) {
    __shared__ __attribute__((aligned(16))) float sh_m[(kBlock / 64) * kHot];
    const uint32_t n = blockIdx.x * static_cast<uint32_t>(kBlock) + threadIdx.x;
    if (n >= static_cast<uint32_t>(C.num_envs)) return;
    float* const sh = sh_m + (threadIdx.x >> 6) * kHot;
    mrac_stage(M, sh);
    const GpdState S{kin, last_rpm, nullptr, step_counter, static_cast<int64_t>(ld32), nullptr, nullptr, nullptr, 0, 0, bad};
    const uint32_t flags = EXT ? C.physics_flags : 0u;
    Lane L;
    L.n = n; L.env = n; L.tid = threadIdx.x; L.le = threadIdx.x; L.d = 0; L.base = threadIdx.x; L.active = true; L.shfl = false;
    Carry c;
    float tgx, tgy, tgz;
    load_carry<false, EXT, false>(S, C, flags, L, kin, nullptr, c, tgx, tgy, tgz, nullptr);     // (no task: a readable dummy target)
    MracState m;
    mrac_load(mst, mld, n * 4u, m);
    int ctr = mcounter[n];
    float4 act = reinterpret_cast<const float4*>(rpm_carry)[n];
    plant_t<PLANT> Q = plant_of<PLANT>(P, plant, S.ld, n * 4u);
    c.roll = c.pitch = c.yaw = 0.0f;
    Tgt tg = load_target(targets, n);
    float rt[4];
    {
        const float r[12] = {tg.a.x, tg.a.y, tg.a.z, tg.a.w, tg.b.x, tg.b.y, tg.b.z, tg.b.w, tg.c.x, tg.c.y, tg.c.z, tg.c.w};
        mrac_rt(mrac_consts(sh), r, rt);
    }
    for (int t = 0; t < K; ++t) {
        // the NEXT step's target row is requested before this step's arithmetic (a held row -- stride 0 -- is read again, a cache
        // hit, and not used)
        const Tgt nx = load_target(targets + (t + 1 < K ? t + 1 : t) * tstride, n);
        StepOut out;
        env_step<false, EXT, false, 4, -1, false>(Q, C, flags, 1, L, act, tgx, tgy, tgz, true, nullptr, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f,
                                                  0.0f, 0.0f, nullptr, nullptr, c, out);
        if (ostride != 0 || t == K - 1)
            store_obs12(obs12 + t * ostride, n, out.o[0], out.o[1], out.o[2], out.o[3], out.o[4], out.o[5], out.o[6], out.o[7],
                        out.o[8], out.o[9], out.o[10], out.o[11]);
        float X[12];
#pragma unroll
        for (int i = 0; i < 9; ++i) X[i] = out.o[i];
        float rpm[4];
        mrac_call(mrac_consts(sh), C.ctrl_dt, X, out.o[9], out.o[10], out.o[11], rt, m, ctr, rpm);
        act = make_float4(rpm[0], rpm[1], rpm[2], rpm[3]);
        if (tstride != 0) {            // (a held target's rt is the same four values every step)
            const float r[12] = {nx.a.x, nx.a.y, nx.a.z, nx.a.w, nx.b.x, nx.b.y, nx.b.z, nx.b.w, nx.c.x, nx.c.y, nx.c.z, nx.c.w};
            mrac_rt(mrac_consts(sh), r, rt);
        }
    }
    store_carry<false>(S, L, c);
    mrac_store(mst, mld, n * 4u, m);
    mcounter[n] = ctr;
    reinterpret_cast<float4*>(rpm_carry)[n] = act;
}

}  // namespace

int gpd_sizeof_mrac(int32_t* size_out) {
    if (!size_out) return Refuse{"gpd_sizeof_mrac"}(GPD_EINVAL, "NULL size_out");
    *size_out = static_cast<int32_t>(sizeof(GpdMrac));
    return 0;
}

int gpd_mrac(const GpdMrac* mrac, float* mrac_state, int32_t* counter, int64_t ld, float ctrl_dt, const float* cur_pos,
             const float* cur_quat, const float* cur_vel, const float* cur_ang_vel, const float* target_pos, const float* target_rpy,
             const float* target_vel, const float* target_rpy_rates, float* rpm, float* pos_e, float* rpy_e, int32_t n, void* stream) {
    const Refuse bad{"gpd_mrac"};
    if (!mrac || !mrac_state || !counter || !cur_pos || !cur_quat || !cur_vel || !cur_ang_vel || !target_pos || !rpm)
        return bad(GPD_EINVAL, "NULL argument");
    if (n <= 0 || ld < n) return bad(GPD_EINVAL, "need 0 < n <= ld");
    if (n > (1 << 26)) return bad(GPD_ERANGE, "more than 2^26 controllers per launch (32-bit byte offsets)");
    if (!(ctrl_dt > 0.0f)) return bad(GPD_EINVAL, "ctrl_dt must be positive");
    if (misaligned16(cur_quat) || misaligned16(rpm)) return bad(GPD_EINVAL, "cur_quat and rpm must be 16-byte aligned");
    hipLaunchKernelGGL(gpd_mrac_kernel, dim3(blocks_for(n, kBlock)), dim3(kBlock), 0, static_cast<hipStream_t>(stream), *mrac, mrac_state, counter, ld,
                       ctrl_dt, cur_pos, cur_quat, cur_vel, cur_ang_vel, target_pos, target_rpy, target_vel, target_rpy_rates, rpm,
                       pos_e, rpy_e, n);
    return launched(bad.who);
}

int gpd_mrac_reset(float* mrac_state, int32_t* counter, int64_t ld, const GpdMrac* mrac, const uint8_t* mask, int32_t n,
                   int32_t restore_gains, void* stream) {
    const Refuse bad{"gpd_mrac_reset"};
    if (!mrac_state || !counter) return bad(GPD_EINVAL, "NULL mrac_state/counter");
    if (restore_gains && !mrac) return bad(GPD_EINVAL, "restore_gains needs the design (NULL mrac)");
    if (n <= 0 || ld < n) return bad(GPD_EINVAL, "need 0 < n <= ld");
    if (n > (1 << 26)) return bad(GPD_ERANGE, "more than 2^26 controllers per launch (32-bit byte offsets)");
    const unsigned blocks = blocks_for(n, kBlock);
    hipStream_t st = static_cast<hipStream_t>(stream);
    hipLaunchKernelGGL(gpd_mrac_reset_kernel, dim3(blocks), dim3(kBlock), 0, st, counter, mask, n);
    if (restore_gains) {
        Gains0 g;
        std::memcpy(g.v, mrac->Kx0, 48 * sizeof(float));
        std::memcpy(g.v + 48, mrac->Kr0, 16 * sizeof(float));
        hipLaunchKernelGGL(gpd_mrac_restore_kernel, dim3(blocks), dim3(kBlock), 0, st, mrac_state, ld, g, mask, n);
    }
    return launched(bad.who);
}

int gpd_rollout_mrac(const GpdParams* params, const GpdMrac* mrac, const GpdState* state, const GpdStepCfg* cfg, float* mrac_state,
                     int32_t* counter, int64_t mrac_ld, const float* targets, int64_t target_step_stride, float* rpm_carry,
                     const float* plant_rows, float* obs12, int64_t obs_step_stride, int32_t num_steps, void* stream) {
    const Refuse bad{"gpd_rollout_mrac"};
    if (!params || !mrac || !state || !cfg) return bad(GPD_EINVAL, "NULL params/mrac/state/cfg");
    if (int rc = check_state(bad, state)) return rc;
    if (!mrac_state || !counter || !targets || !rpm_carry || !obs12) return bad(GPD_EINVAL, "NULL mrac_state/counter/targets/rpm_carry/obs12");
    if (int rc = check_steps(bad, num_steps, target_step_stride, obs_step_stride)) return rc;
    if (int rc = check_flags(bad, cfg)) return rc;
    // what the kernel serves, in front of the remaining shared checks (a configuration outside it answers GPD_ENOTSUP)
    if (cfg->drones_per_env != 1) return bad(GPD_ENOTSUP, "aviaries of one drone only (gpd_step + gpd_mrac serve every shape)");
    if (cfg->task != GPD_TASK_NONE || cfg->auto_reset) return bad(GPD_ENOTSUP, "GPD_TASK_NONE without auto-reset only");
    if (cfg->act_type != GPD_ACT_RAW_RPM && cfg->act_type != GPD_ACT_DIRECT_RPM)
        return bad(GPD_ENOTSUP, "act_type GPD_ACT_RAW_RPM or GPD_ACT_DIRECT_RPM (the controller's output is RPMs)");
    if ((cfg->physics_flags & GPD_PHYS_DW) || state->dw_force) return bad(GPD_ENOTSUP, "downwash needs mates (gpd_step + gpd_mrac)");
    if (int rc = check_positive(bad, cfg)) return rc;
    const int64_t N = cfg->num_envs;
    if (state->ld < N || mrac_ld < N) return bad(GPD_EINVAL, "state.ld / mrac_ld < num_envs");
    if (int rc = check_extent(bad, N, state->ld)) return rc;
    if (int rc = check_needs(bad, params, state, cfg, nullptr, nullptr)) return rc;
    if ((target_step_stride != 0 && target_step_stride < 12 * N) || (obs_step_stride != 0 && obs_step_stride < 12 * N))
        return bad(GPD_EINVAL, "a non-zero step stride must be at least 12*num_envs floats");
    if ((target_step_stride & 3) || (obs_step_stride & 3)) return bad(GPD_EINVAL, "step strides must be multiples of 4 floats (16-byte rows)");
    if (misaligned16(targets) || misaligned16(rpm_carry) || misaligned16(obs12) || misaligned16(plant_rows))
        return bad(GPD_EINVAL, "targets, rpm_carry, obs12 and plant_rows must be 16-byte aligned");
    if (!(cfg->ctrl_dt > 0.0f) || !(cfg->pyb_dt > 0.0f)) return bad(GPD_EINVAL, "pyb_dt and ctrl_dt must be positive");
    GpdStepCfg C = *cfg;
    C.target_per_env = 0; C.init_per_env = 0; C.auto_reset = 0; C.task = GPD_TASK_NONE; C.drones_per_env = 1;
    const bool ext = (C.physics_flags & 31u) != 0;
    const dim3 grid(blocks_for(N, kBlock));
    hipStream_t st = static_cast<hipStream_t>(stream);
    with_ext_plant(ext, plant_rows != nullptr, [&](auto ext_, auto plant_) {
        hipLaunchKernelGGL((gpd_rollout_mrac_kernel<decltype(ext_)::value, decltype(plant_)::value>), grid, dim3(kBlock), 0, st, *params, *mrac,
                           state->kin, state->last_rpm, state->step_counter, state->bad, static_cast<uint32_t>(state->ld), C, mrac_state, counter,
                           mrac_ld, targets, target_step_stride, rpm_carry, plant_rows, obs12, obs_step_stride, num_steps);
    });
    return launched(bad.who);
}
