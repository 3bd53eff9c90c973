// diff_kernels.inc -- the differentiable rollout (pulled into abi.hip; DESIGN.md section 3.12):
//   gpd_rollout_tape_kernel   gpd_rollout / gpd_rollout_plant for single-drone aviaries -- the same load_carry / map_action / env_step /
//                             substep / store_carry code, so the same bits -- that also records, per env step, the 13 kinematic floats
//                             the step started from (the plane layout of GpdState.kin, 52 B per drone-step) and, once, the rpm sum the
//                             drag term of the call's first sub-step saw;
//   gpd_rollout_vjp_kernel    the hand-written reverse sweep: one lane per drone, steps K-1 .. 0.  Per step it reads the taped state, the
//                             action row and the cotangent rows, re-runs the forward sub-steps from the taped state for each sub-step in
//                             reverse (S(S+1)/2 recomputations, no scratch memory, no per-sub-step tape), pushes the adjoint through them
//                             and writes the action gradient of the step.  No atomics: every output word has one writer.
//                             <.., PLANT, GP> (gpd_rollout_vjp_plant, DESIGN.md section 3.13): the same lane also sums the cotangents of
//                             the plant rows it reads, 16 registers, and stores them once after the loop;
//   gpd_plant_derive_vjp_kernel  those cotangents -> the nine scale factors: the transpose of gpd_plant_derive's Jacobian
//                             (plant_derive_vjp.inc, which the host tests compile too).
// The adjoint is that of the function AS EXECUTED: a select differentiates the branch taken (the `turn` test of the quaternion update,
// the gimbal fix-up of quat_to_rpy, the clip of GPD_ACT_RAW_RPM, max(0, .) of the reward).  The cos / sinc polynomials of the quaternion
// exponential are differentiated as the polynomials they are (the exact path beyond |t| = 1 rad as cos / sinc).
// The DSLPID sweep (diff_pid_kernels.inc) stands on the same core, which lives here once: the plane and member-row traffic, the taped
// forwards' lane and stores, rpy_vjp / mat_vjp, outputs_vjp, and the entries' checks and prologues.
#include "plant_derive_vjp.inc"

namespace {

__device__ __forceinline__ float norm_thrust_of(const GpdParams& P) { return P.hover_thrust; }
__device__ __forceinline__ float norm_thrust_of(const PlantParams& P) { return P.norm_thrust; }

// One drone's 13 floats from / to three planes of float4[ld] (P | Q | V, as in GpdState.kin) and the row of body rate z: a block in the
// plane layout (kin_load / kin_store: GpdState.kin, a step of the RPM tape, the cotangent block) or the planes of the DSLPID tape.
__device__ __forceinline__ Kin planes_load(const float* __restrict__ P, const float* __restrict__ Q, const float* __restrict__ V,
                                           const float* __restrict__ wz, uint32_t n) {
    const uint32_t off16 = n * 16u;
    const f4v p = *reinterpret_cast<const f4v*>(reinterpret_cast<const char*>(P) + off16);
    const f4v q = *reinterpret_cast<const f4v*>(reinterpret_cast<const char*>(Q) + off16);
    const f4v v = *reinterpret_cast<const f4v*>(reinterpret_cast<const char*>(V) + off16);
    Kin k;
    k.px = p.x; k.py = p.y; k.pz = p.z; k.wx = p.w;
    k.qx = q.x; k.qy = q.y; k.qz = q.z; k.qw = q.w;
    k.vx = v.x; k.vy = v.y; k.vz = v.z; k.wy = v.w;
    k.wz = *reinterpret_cast<const float*>(reinterpret_cast<const char*>(wz) + n * 4u);
    return k;
}
__device__ __forceinline__ void planes_store(float* __restrict__ P, float* __restrict__ Q, float* __restrict__ V, float* __restrict__ wz,
                                             uint32_t n, const Kin& k) {
    const uint32_t off16 = n * 16u;
    // (opaque copies, as in store_carry: the field reads must not be combined into vector loads of the struct)
    float e0 = k.px, e1 = k.py, e2 = k.pz, e3 = k.wx, e4 = k.qx, e5 = k.qy, e6 = k.qz, e7 = k.qw, e8 = k.vx, e9 = k.vy, e10 = k.vz, e11 = k.wy;
    asm volatile("" : "+v"(e0), "+v"(e1), "+v"(e2), "+v"(e3), "+v"(e4), "+v"(e5), "+v"(e6), "+v"(e7), "+v"(e8), "+v"(e9), "+v"(e10), "+v"(e11));
    const f4v p = {e0, e1, e2, e3}, q = {e4, e5, e6, e7}, v = {e8, e9, e10, e11};
    *reinterpret_cast<f4v*>(reinterpret_cast<char*>(P) + off16) = p;
    *reinterpret_cast<f4v*>(reinterpret_cast<char*>(Q) + off16) = q;
    *reinterpret_cast<f4v*>(reinterpret_cast<char*>(V) + off16) = v;
    *reinterpret_cast<float*>(reinterpret_cast<char*>(wz) + n * 4u) = k.wz;
}
__device__ __forceinline__ Kin kin_load(const float* __restrict__ base, int64_t ld, uint32_t n) {
    return planes_load(base, base + 4 * ld, base + 8 * ld, base + 12 * ld, n);
}
__device__ __forceinline__ void kin_store(float* __restrict__ base, int64_t ld, uint32_t n, const Kin& k) {
    planes_store(base, base + 4 * ld, base + 8 * ld, base + 12 * ld, n, k);
}
// The nine controller members from / to nine rows of float[ld], by name: Pid (GpdState.pid, the DSLPID tape) and GpdDslOutCot (g_pid)
// spell them alike.
template <class M>
__device__ __forceinline__ void members_load(const float* __restrict__ rows, int64_t ld, uint32_t off4, M& s) {
    s.ipx = ld_row(rows, ld, 0, off4); s.ipy = ld_row(rows, ld, 1, off4); s.ipz = ld_row(rows, ld, 2, off4);
    s.lr = ld_row(rows, ld, 3, off4); s.lp = ld_row(rows, ld, 4, off4); s.ly = ld_row(rows, ld, 5, off4);
    s.irx = ld_row(rows, ld, 6, off4); s.iry = ld_row(rows, ld, 7, off4); s.irz = ld_row(rows, ld, 8, off4);
}
template <class M>
__device__ __forceinline__ void members_store(float* __restrict__ rows, int64_t ld, uint32_t off4, const M& s) {
    st_row(rows, ld, 0, off4, s.ipx); st_row(rows, ld, 1, off4, s.ipy); st_row(rows, ld, 2, off4, s.ipz);
    st_row(rows, ld, 3, off4, s.lr); st_row(rows, ld, 4, off4, s.lp); st_row(rows, ld, 5, off4, s.ly);
    st_row(rows, ld, 6, off4, s.irx); st_row(rows, ld, 7, off4, s.iry); st_row(rows, ld, 8, off4, s.irz);
}

// What the two taped forwards share around their loops: the lane of a one-drone aviary, and one step's stores
__device__ __forceinline__ Lane tape_lane(uint32_t N) {
    const uint32_t n_raw = blockIdx.x * kBlock + threadIdx.x;
    Lane L;
    L.tid = threadIdx.x;
    L.active = n_raw < N;
    L.n = L.active ? n_raw : 0u;          // (a lane without a drone computes on drone 0 and stores nothing)
    L.env = L.n; L.le = L.tid; L.d = 0; L.base = L.tid; L.shfl = false;
    return L;
}
__device__ __forceinline__ void tape_step_store(const Lane& L, const StepOut& out, float* __restrict__ obs12, float* __restrict__ reward,
                                                uint8_t* __restrict__ terminated, uint8_t* __restrict__ truncated) {
    if (!L.active) return;
    store_obs12(obs12, L.n, out.o[0], out.o[1], out.o[2], out.o[3], out.o[4], out.o[5], out.o[6], out.o[7],
                out.o[8], out.o[9], out.o[10], out.o[11]);
    reward[L.env] = out.rew;
    terminated[L.env] = static_cast<uint8_t>(out.term ? 1 : 0);
    truncated[L.env] = static_cast<uint8_t>(out.trunc ? 1 : 0);
}

// ------------------------------------------------------------------------------------------------
// the taped forward: K env steps per launch, one lane per drone, state in registers
// ------------------------------------------------------------------------------------------------
template <bool EXT, int AW, bool PLANT>
__global__ __launch_bounds__(kBlock) void gpd_rollout_tape_kernel(const GpdParams P, const GpdState S, const GpdStepCfg C, const int K, const int64_t a_stride,
                                                                  const int64_t o_stride, const int64_t e_stride,
                                                                  const float* __restrict__ actions, const float* __restrict__ target_pos,
                                                                  float* __restrict__ obs12, float* __restrict__ reward,
                                                                  uint8_t* __restrict__ terminated, uint8_t* __restrict__ truncated,
                                                                  const float* __restrict__ plant, float* __restrict__ tape) {
    const Lane L = tape_lane(static_cast<uint32_t>(C.num_envs));
    const uint32_t flags = EXT ? C.physics_flags : 0u;
    const int64_t ld = S.ld;
    Carry c;
    float tgx, tgy, tgz;
    load_carry<false, EXT, false>(S, C, flags, L, target_pos, nullptr, c, tgx, tgy, tgz, nullptr);
    c.roll = c.pitch = c.yaw = 0.0f;
    plant_t<PLANT> Q = plant_of<PLANT>(P, plant, ld, L.n * 4u);
    // the rpm sum the drag term of the call's first sub-step sees: a constant of the reverse sweep (the same expression as env_step's)
    if (L.active) tape[static_cast<int64_t>(K) * 13 * ld + L.n] = ((c.l0 + c.l1) + c.l2) + c.l3;
    for (int t = 0; t < K; ++t, actions += a_stride, obs12 += o_stride, reward += e_stride, terminated += e_stride, truncated += e_stride,
                            tape += 13 * ld) {
        const float4 act = load_action<AW>(actions, L.n);
        if (L.active) kin_store(tape, ld, L.n, c.k);
        StepOut out;
        env_step<false, EXT, false, AW>(Q, C, flags, 1, L, act, tgx, tgy, tgz, false, nullptr, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f,
                                        nullptr, nullptr, c, out);
        tape_step_store(L, out, obs12, reward, terminated, truncated);
    }
    if (L.active) store_carry<false>(S, L, c);
}

// ------------------------------------------------------------------------------------------------
// the reverse sweep
// ------------------------------------------------------------------------------------------------
// Adjoint of quat_to_rpy at (x, y, z, w): (gr, gp, gy) are the cotangents of roll / pitch / yaw, (ax, ay, az, aw) receive the quaternion's.
// Both branches are evaluated and selected (a lane on the branch not taken may compute inf / NaN there, which the select discards):
// a branch that writes through the references makes the caller's cotangent struct an indexed array in scratch memory.
__device__ __forceinline__ void rpy_vjp(float x, float y, float z, float w, float gr, float gp, float gy,
                                        float& ax, float& ay, float& az, float& aw) {
    const float sarg = -2.0f * fmaf(x, z, -(w * y));             // (the expression quat_to_rpy tests)
    const bool gimbal = fabsf(sarg) >= 0.99999f;
    // gimbal branch: roll = 0, pitch = +-pi/2, yaw = 2 atan2(+-x, -+y): d yaw = 2 (x dy - y dx) / (x^2 + y^2) on both signs
    const float inv = 2.0f * gy / fmaf(x, x, y * y);
    const float a_s = 2.0f * gp * fast_rsq((1.0f - sarg) * (1.0f + sarg));      // pitch = asin(sarg), sarg = 2 (w y - x z)
    const float ra = 2.0f * fmaf(y, z, w * x), rb = fmaf(w, w, z * z) - fmaf(x, x, y * y);     // roll = atan2(ra, rb)
    const float ri = gr / fmaf(ra, ra, rb * rb);
    const float a_ra = 2.0f * ri * rb, a_rb = -2.0f * ri * ra;
    const float ya = 2.0f * fmaf(x, y, w * z), yb = fmaf(w, w, -(y * y)) + fmaf(x, x, -(z * z));   // yaw = atan2(ya, yb)
    const float yi = gy / fmaf(ya, ya, yb * yb);
    const float a_ya = 2.0f * yi * yb, a_yb = -2.0f * yi * ya;
    const float rx = (a_ra * w - a_rb * x) + (a_ya * y + a_yb * x) - a_s * z;
    const float ry = (a_ra * z - a_rb * y) + (a_ya * x - a_yb * y) + a_s * w;
    const float rz = (a_ra * y + a_rb * z) + (a_ya * w - a_yb * z) - a_s * x;
    const float rw = (a_ra * x + a_rb * w) + (a_ya * z + a_yb * w) + a_s * y;
    ax = gimbal ? -(inv * y) : rx;
    ay = gimbal ? inv * x : ry;
    az = gimbal ? 0.0f : rz;
    aw = gimbal ? 0.0f : rw;
}

// Adjoint of quat_to_mat at (x, y, z, w): the nine cotangents of R -> += the quaternion's.  R = I + s B(q), s = 2 / |q|^2.
__device__ __forceinline__ void mat_vjp(float x, float y, float z, float w, float r00, float r01, float r02, float r10, float r11, float r12,
                                        float r20, float r21, float r22, float& ax, float& ay, float& az, float& aw) {
    const float d = fmaf(x, x, fmaf(y, y, fmaf(z, z, w * w)));
    const float s = 2.0f / d;
    const float a_s = -(r00 * fmaf(y, y, z * z) + r11 * fmaf(x, x, z * z) + r22 * fmaf(x, x, y * y))
                      + r01 * fmaf(x, y, -(w * z)) + r02 * fmaf(x, z, w * y) + r10 * fmaf(x, y, w * z)
                      + r12 * fmaf(y, z, -(w * x)) + r20 * fmaf(x, z, -(w * y)) + r21 * fmaf(y, z, w * x);
    const float a_d2 = -2.0f * (s / d) * a_s;                   // d s / d q_i = -(s / d) 2 q_i
    const float b00 = s * r00, b01 = s * r01, b02 = s * r02, b10 = s * r10, b11 = s * r11, b12 = s * r12, b20 = s * r20, b21 = s * r21, b22 = s * r22;
    ax += fmaf(a_d2, x, (b01 + b10) * y + (b02 + b20) * z + (b21 - b12) * w - 2.0f * (b11 + b22) * x);
    ay += fmaf(a_d2, y, (b01 + b10) * x + (b12 + b21) * z + (b02 - b20) * w - 2.0f * (b00 + b22) * y);
    az += fmaf(a_d2, z, (b02 + b20) * x + (b12 + b21) * y + (b10 - b01) * w - 2.0f * (b00 + b11) * z);
    aw += fmaf(a_d2, w, (b10 - b01) * z + (b02 - b20) * y + (b21 - b12) * x);
}

// Cotangents of the plant rows the sweep reads (gpd_rollout_vjp_plant), one drone's, in registers for all K steps: the 16 rows of
// include/gpd.h GPD_PLANT_* that the supported configurations read, as named scalars (an indexed member would live in scratch memory).
// NoCot stands in where nobody asks for them: the sweep's code is then what it was.
struct PlantCot {
    float inv_m = 0.0f, gravity = 0.0f, kf = 0.0f, resid = 0.0f, norm_thrust = 0.0f, norm_gap = 0.0f;
    float j0 = 0.0f, j1 = 0.0f, j2 = 0.0f, ji0 = 0.0f, ji1 = 0.0f, ji2 = 0.0f, km_over_kf = 0.0f, d0 = 0.0f, d1 = 0.0f, d2 = 0.0f;
};
struct NoCot {};
template <bool GP> using plant_cot_t = std::conditional_t<GP, PlantCot, NoCot>;

// Adjoint of one physics sub-step (substep<> of gpd_common.inc, the terms this entry supports: thrust, torques, Euler's equation, drag,
// semi-implicit Euler, the exponential quaternion update, the observed world angular velocity).
//   k        the state the sub-step STARTED from (recomputed by the caller)
//   a        in: cotangent of the state it left; out: cotangent of the state it started from
//   b*       AV: cotangent of the observed world angular velocity (pre-update rotation, post-update rates)
//   ag[4]    += cotangent of the rotor thrust deviations;   a_drag  += cotangent of the rpm sum the drag term saw
//   G        GP: += cotangents of the plant rows the sub-step reads (inv_M, GRAVITY, J, J_INV, km_over_kf, the drag coefficients)
template <bool EXT, bool AV, bool GP = false>
__device__ __forceinline__ void substep_vjp(const GpdParams& P, const float h, const uint32_t flags, const float g[4], const float drag_sum,
                                            const Kin& k, Kin& a, const float bx, const float by, const float bz, float ag[4],
                                            float& a_drag, plant_cot_t<GP>& G) {
    const bool drag = EXT && (flags & GPD_PHYS_DRAG);
    // ---- forward: what the reverse pass needs of it
    const Mat3 R = quat_to_mat(k.qx, k.qy, k.qz, k.qw);
    const float dev = ((g[0] + g[1]) + g[2]) + g[3];
    const float T = P.GRAVITY + dev;
    const float wsum = drag ? drag_sum * (6.28318530717958647692f / 60.0f) : 0.0f;
    const float kz = (P.drone_model == GPD_MODEL_RACE) ? -P.km_over_kf : P.km_over_kf;
    const float gz = ((-g[0] + g[1]) - g[2]) + g[3];
    const float tz = kz * gz;
    const float arm = P.L * 0.70710678118654752440f;
    const float arm_x = (P.drone_model == GPD_MODEL_CF2X) ? -arm : arm;
    const bool plus = P.drone_model == GPD_MODEL_CF2P;
    const float tx = plus ? (g[1] - g[3]) * P.L : (((g[0] + g[1]) - g[2]) - g[3]) * arm_x;
    const float ty = plus ? (-g[0] + g[2]) * P.L : (((-g[0] + g[1]) + g[2]) - g[3]) * arm;
    const float jwx = P.J[0] * k.wx, jwy = P.J[1] * k.wy, jwz = P.J[2] * k.wz;
    const float tqx = tx - fmaf(k.wy, jwz, -(k.wz * jwy));
    const float tqy = ty - fmaf(k.wz, jwx, -(k.wx * jwz));
    const float tqz = tz - fmaf(k.wx, jwy, -(k.wy * jwx));
    const float wx = fmaf(h, P.J_INV[0] * tqx, k.wx), wy = fmaf(h, P.J_INV[1] * tqy, k.wy), wz = fmaf(h, P.J_INV[2] * tqz, k.wz);   // new rates
    const float n2 = fmaf(wz, wz, fmaf(wy, wy, wx * wx));
    const float u = n2 * (0.25f * h * h);
    // cos t and sin t / t as substep<>'s polynomials in u = t^2, and their derivatives in u
    float cs = fmaf(fmaf(fmaf(fmaf(2.412107309e-05f, u, -1.388295778e-03f), u, 4.166645522e-02f), u, -4.999999736e-01f), u, 9.999999995e-01f);
    float sp = fmaf(fmaf(fmaf(fmaf(2.693749890e-06f, u, -1.983586443e-04f), u, 8.333314057e-03f), u, -1.666666643e-01f), u, 1.0f);
    float dcs = fmaf(fmaf(fmaf(4.0f * 2.412107309e-05f, u, 3.0f * -1.388295778e-03f), u, 2.0f * 4.166645522e-02f), u, -4.999999736e-01f);
    float dsp = fmaf(fmaf(fmaf(4.0f * 2.693749890e-06f, u, 3.0f * -1.983586443e-04f), u, 2.0f * 8.333314057e-03f), u, -1.666666643e-01f);
    if (!(u <= 1.0f)) {                    // tumbling: substep<>'s exact path, d cos(sqrt u) / du = -sinc / 2, d sinc / du = (cos - sinc) / 2u
        const float n = sqrtf(n2);
        float sn;
        sincosf(n * h * 0.5f, &sn, &cs);
        sp = sn / (n * h * 0.5f);
        dcs = -0.5f * sp;
        dsp = 0.5f * (cs - sp) / u;
    }
    const float sc = sp * (0.5f * h);
    const bool turn = n2 > 1e-16f;

    // ---- reverse
    float awx = a.wx, awy = a.wy, awz = a.wz;                  // cotangent of the NEW rates
    if (AV) {                                                  // av = R w'
        awx += fmaf(R.r00, bx, fmaf(R.r10, by, R.r20 * bz));
        awy += fmaf(R.r01, bx, fmaf(R.r11, by, R.r21 * bz));
        awz += fmaf(R.r02, bx, fmaf(R.r12, by, R.r22 * bz));
    }
    float aqx = a.qx, aqy = a.qy, aqz = a.qz, aqw = a.qw;      // becomes the cotangent of the OLD quaternion
    if (turn) {                                                // q' = cs q + sc (q (x) [w', 0])
        const float lx = fmaf(wx, k.qw, fmaf(wz, k.qy, -(wy * k.qz)));
        const float ly = fmaf(wy, k.qw, fmaf(wx, k.qz, -(wz * k.qx)));
        const float lz = fmaf(wz, k.qw, fmaf(wy, k.qx, -(wx * k.qy)));
        const float lw = -fmaf(wz, k.qz, fmaf(wy, k.qy, wx * k.qx));
        const float a_cs = fmaf(a.qx, k.qx, fmaf(a.qy, k.qy, fmaf(a.qz, k.qz, a.qw * k.qw)));
        const float a_sc = fmaf(a.qx, lx, fmaf(a.qy, ly, fmaf(a.qz, lz, a.qw * lw)));
        const float alx = sc * a.qx, aly = sc * a.qy, alz = sc * a.qz, alw = sc * a.qw;
        aqx = fmaf(cs, a.qx, (alz * wy - aly * wz) - alw * wx);
        aqy = fmaf(cs, a.qy, (alx * wz - alz * wx) - alw * wy);
        aqz = fmaf(cs, a.qz, (aly * wx - alx * wy) - alw * wz);
        aqw = fmaf(cs, a.qw, fmaf(alx, wx, fmaf(aly, wy, alz * wz)));
        const float a_n2 = fmaf(a_cs, dcs, a_sc * (0.5f * h) * dsp) * (0.25f * h * h);
        awx += ((alx * k.qw + aly * k.qz) - alz * k.qy) - alw * k.qx + 2.0f * wx * a_n2;
        awy += ((aly * k.qw - alx * k.qz) + alz * k.qx) - alw * k.qy + 2.0f * wy * a_n2;
        awz += ((alx * k.qy - aly * k.qx) + alz * k.qw) - alw * k.qz + 2.0f * wz * a_n2;
    }
    // p' = p + h v': the position's cotangent passes through
    const float avx = fmaf(h, a.px, a.vx), avy = fmaf(h, a.py, a.vy), avz = fmaf(h, a.pz, a.vz);    // cotangent of the NEW velocity
    // w' = w + h J^-1 (t - w x J w)
    const float atx = h * P.J_INV[0] * awx, aty = h * P.J_INV[1] * awy, atz = h * P.J_INV[2] * awz;
    const float j21 = P.J[2] - P.J[1], j02 = P.J[0] - P.J[2], j10 = P.J[1] - P.J[0];
    a.wx = awx - fmaf(aty, k.wz * j02, atz * (k.wy * j10));
    a.wy = awy - fmaf(atx, k.wz * j21, atz * (k.wx * j10));
    a.wz = awz - fmaf(atx, k.wy * j21, aty * (k.wx * j02));
    if constexpr (GP) {
        // w'_i = w_i + h J_INV[i] tq_i;  tq = t - w x (J w), J w row by row;  tz = +-km_over_kf (-g0 + g1 - g2 + g3)
        G.ji0 = fmaf(h * tqx, awx, G.ji0); G.ji1 = fmaf(h * tqy, awy, G.ji1); G.ji2 = fmaf(h * tqz, awz, G.ji2);
        G.j0 = fmaf(fmaf(atz, k.wy, -(aty * k.wz)), k.wx, G.j0);
        G.j1 = fmaf(fmaf(atx, k.wz, -(atz * k.wx)), k.wy, G.j1);
        G.j2 = fmaf(fmaf(aty, k.wx, -(atx * k.wy)), k.wz, G.j2);
        const float a_kz = atz * gz;
        G.km_over_kf += (P.drone_model == GPD_MODEL_RACE) ? -a_kz : a_kz;
    }
    const float kzt = kz * atz;
    ag[0] -= kzt; ag[1] += kzt; ag[2] -= kzt; ag[3] += kzt;
    if (plus) {
        ag[1] += P.L * atx; ag[3] -= P.L * atx; ag[0] -= P.L * aty; ag[2] += P.L * aty;
    } else {
        const float px_ = arm_x * atx, py_ = arm * aty;
        ag[0] += px_ - py_; ag[1] += px_ + py_; ag[2] += py_ - px_; ag[3] -= px_ + py_;
    }
    // v' = v + h F / M
    const float afx = h * P.inv_M * avx, afy = h * P.inv_M * avy, afz = h * P.inv_M * avz;
    a.vx = avx; a.vy = avy; a.vz = avz;
    if (drag) {                                                // F -= drag_coeff * v * wsum
        a.vx = fmaf(-(P.drag_coeff[0] * wsum), afx, a.vx);
        a.vy = fmaf(-(P.drag_coeff[1] * wsum), afy, a.vy);
        a.vz = fmaf(-(P.drag_coeff[2] * wsum), afz, a.vz);
        const float a_wsum = -fmaf(P.drag_coeff[0] * k.vx, afx, fmaf(P.drag_coeff[1] * k.vy, afy, (P.drag_coeff[2] * k.vz) * afz));
        a_drag += a_wsum * (6.28318530717958647692f / 60.0f);
    }
    if constexpr (GP) {
        // v' = v + h inv_M F: the force as substep<> assembles it (F_z from the deviation, 1 - R22 computed directly)
        float Fx = R.r02 * T, Fy = R.r12 * T, Fz = fmaf(R.r22, dev, -(P.GRAVITY * R.m22));
        if (drag) {
            Fx = fmaf(-(P.drag_coeff[0] * k.vx), wsum, Fx);
            Fy = fmaf(-(P.drag_coeff[1] * k.vy), wsum, Fy);
            Fz = fmaf(-(P.drag_coeff[2] * k.vz), wsum, Fz);
            G.d0 = fmaf(-(k.vx * wsum), afx, G.d0);
            G.d1 = fmaf(-(k.vy * wsum), afy, G.d1);
            G.d2 = fmaf(-(k.vz * wsum), afz, G.d2);
        }
        G.inv_m = fmaf(h, fmaf(Fx, avx, fmaf(Fy, avy, Fz * avz)), G.inv_m);
        // GRAVITY twice: in T = GRAVITY + sum g (the cotangent of T) and in -GRAVITY e_z; together afx R02 + afy R12 - afz (1 - R22)
        G.gravity += fmaf(afx, R.r02, fmaf(afy, R.r12, -(afz * R.m22)));
    }
    // F = R[:, 2] T - (0, 0, GRAVITY)
    const float a_T = fmaf(afx, R.r02, fmaf(afy, R.r12, afz * R.r22));
    ag[0] += a_T; ag[1] += a_T; ag[2] += a_T; ag[3] += a_T;
    // cotangent of the rotation matrix: the force column, and (AV) the observed angular velocity
    const float r02 = fmaf(afx, T, AV ? bx * wz : 0.0f), r12 = fmaf(afy, T, AV ? by * wz : 0.0f), r22 = fmaf(afz, T, AV ? bz * wz : 0.0f);
    const float r00 = AV ? bx * wx : 0.0f, r01 = AV ? bx * wy : 0.0f, r10 = AV ? by * wx : 0.0f, r11 = AV ? by * wy : 0.0f;
    const float r20 = AV ? bz * wx : 0.0f, r21 = AV ? bz * wy : 0.0f;
    a.qx = aqx; a.qy = aqy; a.qz = aqz; a.qw = aqw;
    mat_vjp(k.qx, k.qy, k.qz, k.qw, r00, r01, r02, r10, r11, r12, r20, r21, r22, a.qx, a.qy, a.qz, a.qw);
}

// Adjoint of map_action<false, AW> (the four RPM action types): out[AW] = cotangent of the raw action row
//   ag[4]  cotangent of the thrust deviations;  a_sum  cotangent of the step's rpm sum (what the drag terms saw of it)
//   G      GP: += cotangents of the plant rows the mapping reads: norm_thrust and norm_gap (g = norm_thrust e (2 + e) - norm_gap), or
//          KF and hover_resid (g = KF (rpm - h)(rpm + h) + hover_resid, at the CLIPPED rpm: a rotor outside the clip still has a thrust)
template <int AW, bool GP = false, class PP>
__device__ __forceinline__ void action_vjp(const PP& P, const GpdStepCfg& C, const float4 act, const float rpm[4], const float ag[4],
                                           const float a_sum, float out[4], plant_cot_t<GP>& G) {
    const float nt = norm_thrust_of(P);
    if (AW == 1) {                        // one value drives the four rotors
        const float e = 0.05f * act.x;
        const float ag_sum = ((ag[0] + ag[1]) + ag[2]) + ag[3];
        out[0] = 0.05f * fmaf(ag_sum, nt * (2.0f + 2.0f * e), 4.0f * a_sum * P.hover_rpm);
        out[1] = out[2] = out[3] = 0.0f;
        if constexpr (GP) {
            G.norm_thrust = fmaf(ag_sum, e * (2.0f + e), G.norm_thrust);
            G.norm_gap -= ag_sum;
        }
    } else if (C.act_type == GPD_ACT_RPM) {
        const float av[4] = {act.x, act.y, act.z, act.w};
#pragma unroll
        for (int i = 0; i < 4; ++i) out[i] = 0.05f * fmaf(ag[i], nt * (2.0f + 2.0f * (0.05f * av[i])), a_sum * P.hover_rpm);
        if constexpr (GP) {
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                const float e = 0.05f * av[i];
                G.norm_thrust = fmaf(ag[i], e * (2.0f + e), G.norm_thrust);
            }
            G.norm_gap -= ((ag[0] + ag[1]) + ag[2]) + ag[3];
        }
    } else {                              // RAW_RPM: zero outside the clip; DIRECT_RPM: as is
        const bool clip = C.act_type == GPD_ACT_RAW_RPM;
        const float av[4] = {act.x, act.y, act.z, act.w};
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const bool inside = !clip || (av[i] >= 0.0f && av[i] <= P.max_rpm);
            out[i] = inside ? fmaf(ag[i], 2.0f * P.KF * rpm[i], a_sum) : 0.0f;
        }
        if constexpr (GP) {
#pragma unroll
            for (int i = 0; i < 4; ++i) G.kf = fmaf(ag[i], (rpm[i] - P.hover_rpm) * (rpm[i] + P.hover_rpm), G.kf);
            G.resid += ((ag[0] + ag[1]) + ag[2]) + ag[3];
        }
    }
}

// The step's outputs are functions of the state kp its LAST sub-step leaves: obs12 = pos | rpy | vel | ang_v, the reward.  A += the
// cotangents of pos, rpy, vel (go[0..8]) and of the reward (grew); that of ang_v (go[9..11]) goes through substep_vjp<.., AV = true>.
__device__ __forceinline__ void outputs_vjp(const Kin& kp, const float go[12], const float grew, const float tgx, const float tgy,
                                            const float tgz, Kin& A) {
    A.px += go[0]; A.py += go[1]; A.pz += go[2];
    A.vx += go[6]; A.vy += go[7]; A.vz += go[8];
    float rqx, rqy, rqz, rqw;
    rpy_vjp(kp.qx, kp.qy, kp.qz, kp.qw, go[3], go[4], go[5], rqx, rqy, rqz, rqw);
    A.qx += rqx; A.qy += rqy; A.qz += rqz; A.qw += rqw;
    {   // reward = max(0, 2 - |target - p|^4), task_single's expressions
        const float ex = tgx - kp.px, ey = tgy - kp.py, ez = tgz - kp.pz;
        const float dist = fast_sqrt(fmaf(ez, ez, fmaf(ey, ey, ex * ex)));
        const float dd = dist * dist;
        const float gr = fmaf(-dd, dd, 2.0f) > 0.0f ? 4.0f * dd * grew : 0.0f;
        A.px = fmaf(gr, ex, A.px); A.py = fmaf(gr, ey, A.py); A.pz = fmaf(gr, ez, A.pz);
    }
}

// GP (only with PLANT): the lane also accumulates the cotangents of its drone's plant rows over the whole sweep and stores them once,
// after the loop, into g_plant [GPD_PLANT_ROWS][ld] -- rows no supported configuration reads as exactly 0.  g_plant is NULL otherwise.
template <bool EXT, int AW, bool PLANT, bool GP = false>
__global__ __launch_bounds__(kBlock) void gpd_rollout_vjp_kernel(const GpdParams P, const GpdStepCfg C, const int64_t ld, const int K,
                                                                 const float* __restrict__ actions, const int64_t a_stride,
                                                                 const float* __restrict__ target_pos, const float* __restrict__ plant,
                                                                 const float* __restrict__ tape, const float* __restrict__ g_obs12,
                                                                 const int64_t o_stride, const float* __restrict__ g_reward,
                                                                 const int64_t e_stride, float* __restrict__ g_kin,
                                                                 float* __restrict__ g_actions, float* __restrict__ g_plant) {
    static_assert(PLANT || !GP, "the plant rows' cotangents need a plant table");
    const uint32_t N = static_cast<uint32_t>(C.num_envs);
    const uint32_t n = blockIdx.x * kBlock + threadIdx.x;
    if (n >= N) return;
    const uint32_t flags = EXT ? C.physics_flags : 0u;
    const bool drag = EXT && (flags & GPD_PHYS_DRAG);
    plant_t<PLANT> Q = plant_of<PLANT>(P, plant, ld, n * 4u);
    const bool has_task = C.task != GPD_TASK_NONE;
    const float* tp = target_pos + (C.target_per_env ? static_cast<size_t>(n) * 3 : 0);      // (task NONE: a readable dummy)
    const float tgx = tp[0], tgy = tp[1], tgz = tp[2];
    const float h = C.pyb_dt;
    const int S = C.substeps;
    Kin A = kin_load(g_kin, ld, n);                         // cotangent of the state after the step in hand
    float a_next = 0.0f;                                       // cotangent of this step's rpm sum from the NEXT step's first drag term
    plant_cot_t<GP> G;                                         // GP: cotangents of the plant rows, summed over the sweep
    const float first_sum = drag ? tape[static_cast<int64_t>(K) * 13 * ld + n] : 0.0f;
    for (int t = K - 1; t >= 0; --t) {
        const Kin k0 = kin_load(tape + static_cast<int64_t>(t) * 13 * ld, ld, n);
        const float4 act = load_action<AW>(actions + t * a_stride, n);
        Carry c{};
        c.k = k0;
        float rpm[4], g[4];
        map_action<false, AW, -1>(Q, C, act, c, rpm, g);
        const float cur_sum = ((rpm[0] + rpm[1]) + rpm[2]) + rpm[3];
        float prev_sum = cur_sum;
        if (drag) {                                            // the first sub-step sees the previous step's RPMs
            prev_sum = first_sum;
            if (t > 0) {
                float rp[4], gp_[4];
                map_action<false, AW, -1>(Q, C, load_action<AW>(actions + (t - 1) * a_stride, n), c, rp, gp_);
                prev_sum = ((rp[0] + rp[1]) + rp[2]) + rp[3];
            }
        }
        // (This load and the loop over the sub-steps below stand in gpd_rollout_vjp_pid_kernel too: shared, the load in three forms cost
        // 1 - 4 % of the sweeps' time, the loop 1 - 6 VGPRs as one function and 1.3 % at S = 8 with its body alone shared.)
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
        float ag[4] = {0.0f, 0.0f, 0.0f, 0.0f};
        float a_cur = a_next, a_prev = 0.0f;
        float d0, d1, d2;
        for (int j = S - 1; j >= 0; --j) {
            Kin k = k0;                                        // the state sub-step j started from: j forward sub-steps from the tape
            for (int i = 0; i < j; ++i) substep<EXT, false>(Q, h, flags, g, i == 0 ? prev_sum : cur_sum, 0.0f, k, d0, d1, d2);
            const float ds = j == 0 ? prev_sum : cur_sum;
            float a_drag = 0.0f;
            if (j == S - 1) {
                // the step's outputs are functions of the state its LAST sub-step leaves: obs12 = pos | rpy | vel | ang_v, the reward
                Kin kp = k;
                substep<EXT, false>(Q, h, flags, g, ds, 0.0f, kp, d0, d1, d2);
                outputs_vjp(kp, go, grew, tgx, tgy, tgz, A);
                substep_vjp<EXT, true, GP>(Q, h, flags, g, ds, k, A, go[9], go[10], go[11], ag, a_drag, G);
            } else {
                substep_vjp<EXT, false, GP>(Q, h, flags, g, ds, k, A, 0.0f, 0.0f, 0.0f, ag, a_drag, G);
            }
            a_prev += j == 0 ? a_drag : 0.0f;                  // (selects: a branch here makes the two sums an indexed array in scratch)
            a_cur += j == 0 ? 0.0f : a_drag;
        }
        float ga[4];
        action_vjp<AW, GP>(Q, C, act, rpm, ag, a_cur, ga, G);
        float* dst = g_actions + (static_cast<size_t>(t) * N + n) * AW;
        if (AW == 4) *reinterpret_cast<f4v*>(dst) = f4v{ga[0], ga[1], ga[2], ga[3]};
        else dst[0] = ga[0];
        a_next = a_prev;
    }
    kin_store(g_kin, ld, n, A);
    if constexpr (GP) {
        const float rows[GPD_PLANT_ROWS] = {0.0f /* M */, G.inv_m, G.kf, G.gravity, G.j0, G.j1, G.j2, G.ji0, G.ji1, G.ji2, G.km_over_kf,
                                            0.0f /* GND_EFF */, G.d0, G.d1, G.d2, 0.0f /* HOVER_THRUST */, G.resid, G.norm_thrust, G.norm_gap};
#pragma unroll
        for (int r = 0; r < GPD_PLANT_ROWS; ++r) st_row(g_plant, ld, r, n * 4u, rows[r]);
    } else {
        (void)g_plant;
    }
}

// gpd_plant_derive_vjp: one lane per drone, the transpose of gpd_plant_derive_kernel's Jacobian at the drone's scales -- the formulas of
// plant_derive_vjp.inc in float64 from the fp32 inputs, one rounding per output, as the derivation itself.
__global__ __launch_bounds__(256) void gpd_plant_derive_vjp_kernel(const GpdParams P, const float* __restrict__ scales,
                                                                   const float* __restrict__ g_rows, const uint32_t n, const int64_t ld,
                                                                   float* __restrict__ g_scales) {
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (i >= n) return;
    double s[GPD_NUM_SCALES], g[GPD_PLANT_ROWS], out[GPD_NUM_SCALES];
#pragma unroll
    for (int k = 0; k < GPD_NUM_SCALES; ++k) s[k] = scales[k * ld + i];
#pragma unroll
    for (int r = 0; r < GPD_PLANT_ROWS; ++r) g[r] = g_rows[r * ld + i];
    gpd_plant_derive_vjp_one(&P, s, g, out);
#pragma unroll
    for (int k = 0; k < GPD_NUM_SCALES; ++k) g_scales[k * ld + i] = static_cast<float>(out[k]);
}

// What the entries of the rollout check of the configuration and refuse of it, before any device work: the span and the sizes, then what is
// not differentiable in the family the entry serves (the RPM action types of this file, the DSLPID ones of diff_pid_kernels.inc, or the
// thrust-and-body-rate loop of diff_ctbr_kernels.inc, which narrows the configuration as gpd_rollout_ctbr does).
// `ld` comes without the state in two entries of each family.
enum class DiffFamily { RPM, PID, CTBR };
int diff_cfg(Refuse bad, DiffFamily family, const GpdStepCfg* cfg, int64_t ld, int32_t num_steps, int64_t stride0 = 0, int64_t stride1 = 0,
             int64_t stride2 = 0) {
    if (int rc = check_steps(bad, num_steps, stride0, stride1, stride2)) return rc;
    if (int rc = check_ranges(bad, cfg)) return rc;
    if (int rc = check_positive(bad, cfg)) return rc;
    if (int rc = check_flags(bad, cfg)) return rc;
    if (ld <= 0 || ld > 0xffffffffLL) return bad(GPD_EINVAL, "ld must be in 1 .. 2^32 - 1 (floats)");
    if (int rc = check_extent(bad, static_cast<int64_t>(cfg->num_envs) * cfg->drones_per_env, ld, "ld")) return rc;
    if (cfg->drones_per_env != 1) return bad(GPD_ENOTSUP, "aviaries of more than one drone are not differentiable (drones_per_env must be 1)");
    if (cfg->task != GPD_TASK_NONE && cfg->task != GPD_TASK_HOVER) return bad(GPD_ENOTSUP, "task must be GPD_TASK_NONE or GPD_TASK_HOVER");
    if (family == DiffFamily::RPM) {
        if (cfg->act_type != GPD_ACT_RPM && cfg->act_type != GPD_ACT_ONE_D_RPM && cfg->act_type != GPD_ACT_RAW_RPM && cfg->act_type != GPD_ACT_DIRECT_RPM)
            return bad(GPD_ENOTSUP, "the DSLPID action types are not differentiable (RPM, ONE_D_RPM, RAW_RPM and DIRECT_RPM are)");
        if (cfg->physics_flags & ~static_cast<uint32_t>(GPD_PHYS_DRAG))
            return bad(GPD_ENOTSUP, "physics_flags other than GPD_PHYS_DRAG are not differentiable (ground effect, downwash, ground plane, damping)");
    } else if (family == DiffFamily::CTBR) {
        if (cfg->task != GPD_TASK_NONE) return bad(GPD_ENOTSUP, "GPD_TASK_NONE without auto-reset only");
        if (cfg->act_type != GPD_ACT_RAW_RPM && cfg->act_type != GPD_ACT_DIRECT_RPM)
            return bad(GPD_ENOTSUP, "act_type GPD_ACT_RAW_RPM or GPD_ACT_DIRECT_RPM (the rate loop's output is RPMs)");
        if (cfg->physics_flags)
            return bad(GPD_ENOTSUP, "physics_flags are not differentiable together with the body-rate loop (ground effect, drag -- its rpm sum has "
                                    "no derivative at a rotor held at 0 --, downwash, ground plane, damping)");
    } else {
        if (cfg->act_type != GPD_ACT_PID && cfg->act_type != GPD_ACT_VEL && cfg->act_type != GPD_ACT_ONE_D_PID)
            return bad(GPD_ENOTSUP, "the RPM action types go through gpd_rollout_tape / gpd_rollout_vjp (this entry: PID, VEL and ONE_D_PID)");
        if (cfg->physics_flags)
            return bad(GPD_ENOTSUP, "physics_flags are not differentiable together with DSLPID (drag, ground effect, downwash, ground plane, damping)");
    }
    if (cfg->auto_reset) return bad(GPD_ENOTSUP, "auto_reset inside a differentiated call is not supported");
    return 0;
}

// The size query of a family's tape: per_step x num_steps + extra rows of ld floats
int tape_floats_impl(Refuse bad, DiffFamily family, const GpdStepCfg* cfg, int32_t num_steps, int64_t ld, int per_step, int extra, int64_t* floats_out) {
    if (!cfg || !floats_out) return bad(GPD_EINVAL, "NULL cfg/floats_out");
    if (int rc = diff_cfg(bad, family, cfg, ld, num_steps)) return rc;
    const int64_t rows = per_step * static_cast<int64_t>(num_steps) + extra;
    if (rows > INT64_MAX / ld) return bad(GPD_ERANGE, "the tape does not fit 2^63 floats");
    *floats_out = rows * ld;
    return 0;
}

// The argument checks of a taped forward (gpd_rollout_tape, gpd_rollout_tape_pid) up to the tape's alignment, then the copies the kernel
// gets: `c` with a readable dummy target where there is no task, `s` without the action ring.
int tape_prologue(Refuse bad, DiffFamily family, const GpdParams* params, const GpdState* state, const GpdStepCfg* cfg, int32_t num_steps,
                  const float* actions, int64_t action_step_stride, const float*& target_pos, const float* obs12, int64_t obs_step_stride,
                  const float* reward, const uint8_t* terminated, const uint8_t* truncated, int64_t env_step_stride, const float* tape,
                  GpdStepCfg& c, GpdState& s) {
    if (!params || !state || !cfg) return bad(GPD_EINVAL, "NULL params/state/cfg");
    if (int rc = check_state(bad, state)) return rc;
    if (!actions || !obs12 || !reward || !terminated || !truncated || !tape)
        return bad(GPD_EINVAL, "NULL actions/obs12/reward/terminated/truncated/tape");
    if (int rc = diff_cfg(bad, family, cfg, state->ld, num_steps, action_step_stride, obs_step_stride, env_step_stride)) return rc;
    if (state->dw_force) return bad(GPD_ENOTSUP, "state.dw_force (downwash computed outside the kernel) is not differentiable");
    if (int rc = check_needs(bad, params, state, cfg, target_pos, nullptr)) return rc;
    if (misaligned16(tape)) return bad(GPD_EINVAL, "tape must be 16-byte aligned");
    c = *cfg;
    s = *state;
    s.act_ring = nullptr;                                      // (a rollout never pushes into the action ring itself)
    dummy_target(c, target_pos, state->kin);
    return 0;
}

// The checks the reverse sweeps (gpd_rollout_vjp / _plant, gpd_rollout_vjp_pid) share after their own NULL lists: the configuration, what
// it needs, the alignment of the two blocks both read as float4.  Each entry goes on with the alignment of its own arguments.
int sweep_prologue(Refuse bad, DiffFamily family, const GpdParams* params, const GpdStepCfg* cfg, int64_t ld, int32_t num_steps,
                   int64_t action_step_stride, int64_t obs_step_stride, int64_t env_step_stride, const float* target_pos,
                   const float* tape, const float* g_kin) {
    if (int rc = diff_cfg(bad, family, cfg, ld, num_steps, action_step_stride, obs_step_stride, env_step_stride)) return rc;
    if (int rc = check_needs(bad, params, nullptr, cfg, target_pos, nullptr)) return rc;
    if (misaligned16(tape) || misaligned16(g_kin)) return bad(GPD_EINVAL, "tape and g_kin must be 16-byte aligned");
    return 0;
}

// act_type -> the action row's width, then <EXT, PLANT>: every kernel of this file is launched as launch(ext, aw, plant)
template <class F>
void diff_dispatch(const GpdStepCfg& c, bool plant, F&& launch) {
    with_ext_plant(c.physics_flags != 0, plant, [&](auto ext, auto pl) {
        if (c.act_type == GPD_ACT_ONE_D_RPM) launch(ext, Const<1>{}, pl); else launch(ext, Const<4>{}, pl);
    });
}

// argument checks + launch shared by gpd_rollout_vjp and gpd_rollout_vjp_plant (g_plant: the plant rows' cotangents, or NULL)
int vjp_impl(Refuse bad, const GpdParams* params, const GpdStepCfg* cfg, int64_t ld, int32_t num_steps, const float* actions,
             int64_t action_step_stride, const float* target_pos, const float* plant_rows, const float* tape, const float* g_obs12,
             int64_t obs_step_stride, const float* g_reward, int64_t env_step_stride, float* g_kin, float* g_actions, float* g_plant,
             void* stream) {
    if (!params || !cfg) return bad(GPD_EINVAL, "NULL params/cfg");
    if (!actions || !tape || !g_kin || !g_actions) return bad(GPD_EINVAL, "NULL actions/tape/g_kin/g_actions");
    if (int rc = sweep_prologue(bad, DiffFamily::RPM, params, cfg, ld, num_steps, action_step_stride, obs_step_stride, env_step_stride,
                                target_pos, tape, g_kin))
        return rc;
    if (misaligned16(plant_rows)) return bad(GPD_EINVAL, "plant_rows must be 16-byte aligned");
    if (misaligned16(g_actions)) return bad(GPD_EINVAL, "g_actions must be 16-byte aligned");
    GpdStepCfg c = *cfg;
    dummy_target(c, target_pos, tape);
    const dim3 grid(blocks_for(c.num_envs, kBlock));
    diff_dispatch(c, plant_rows != nullptr, [&](auto ext, auto aw, auto pl) {
        constexpr bool EXT = decltype(ext)::value, PLANT = decltype(pl)::value;
        constexpr int AW = decltype(aw)::value;
        auto launch = [&](auto gp) {
            hipLaunchKernelGGL((gpd_rollout_vjp_kernel<EXT, AW, PLANT, decltype(gp)::value>), grid, dim3(kBlock), 0,
                               static_cast<hipStream_t>(stream), *params, c, ld, num_steps, actions, action_step_stride, target_pos,
                               plant_rows, tape, g_obs12, obs_step_stride, g_reward, env_step_stride, g_kin, g_actions, g_plant);
        };
        if constexpr (PLANT) {
            if (g_plant) return launch(Const<true>{});
        }
        launch(Const<false>{});
    });
    return launched(bad.who);
}

}  // namespace

extern "C" {

int gpd_rollout_tape_floats(const GpdStepCfg* cfg, int32_t num_steps, int64_t ld, int64_t* floats_out) {
    // 13 per env step + the first drag term's rpm sum
    return tape_floats_impl(Refuse{"gpd_rollout_tape_floats"}, DiffFamily::RPM, cfg, num_steps, ld, 13, 1, floats_out);
}

int gpd_rollout_tape(const GpdParams* params, const GpdState* state, const GpdStepCfg* cfg, int32_t num_steps, const float* actions,
                     int64_t action_step_stride, const float* target_pos, float* obs12, int64_t obs_step_stride, float* reward,
                     uint8_t* terminated, uint8_t* truncated, int64_t env_step_stride, const float* plant_rows, float* tape, void* stream) {
    const Refuse bad{"gpd_rollout_tape"};
    GpdStepCfg c;
    GpdState s;
    if (int rc = tape_prologue(bad, DiffFamily::RPM, params, state, cfg, num_steps, actions, action_step_stride, target_pos, obs12,
                               obs_step_stride, reward, terminated, truncated, env_step_stride, tape, c, s))
        return rc;
    if (misaligned16(plant_rows)) return bad(GPD_EINVAL, "plant_rows must be 16-byte aligned");
    const dim3 grid(blocks_for(c.num_envs, kBlock));
    diff_dispatch(c, plant_rows != nullptr, [&](auto ext, auto aw, auto pl) {
        hipLaunchKernelGGL((gpd_rollout_tape_kernel<decltype(ext)::value, decltype(aw)::value, decltype(pl)::value>), grid, dim3(kBlock), 0,
                           static_cast<hipStream_t>(stream), *params, s, c, num_steps, action_step_stride, obs_step_stride, env_step_stride, actions, target_pos, obs12, reward, terminated, truncated,
                           plant_rows, tape);
    });
    return launched(bad.who);
}

int gpd_rollout_vjp(const GpdParams* params, const GpdStepCfg* cfg, int64_t ld, int32_t num_steps, const float* actions,
                    int64_t action_step_stride, const float* target_pos, const float* plant_rows, const float* tape,
                    const float* g_obs12, int64_t obs_step_stride, const float* g_reward, int64_t env_step_stride, float* g_kin,
                    float* g_actions, void* stream) {
    return vjp_impl(Refuse{"gpd_rollout_vjp"}, params, cfg, ld, num_steps, actions, action_step_stride, target_pos, plant_rows, tape, g_obs12,
                    obs_step_stride, g_reward, env_step_stride, g_kin, g_actions, nullptr, stream);
}

int gpd_rollout_vjp_plant(const GpdParams* params, const GpdStepCfg* cfg, int64_t ld, int32_t num_steps, const float* actions,
                          int64_t action_step_stride, const float* target_pos, const float* plant_rows, const float* tape,
                          const float* g_obs12, int64_t obs_step_stride, const float* g_reward, int64_t env_step_stride, float* g_kin,
                          float* g_actions, float* g_plant_rows, void* stream) {
    const Refuse bad{"gpd_rollout_vjp_plant"};
    if (!plant_rows || !g_plant_rows) return bad(GPD_EINVAL, "NULL plant_rows/g_plant_rows (the plant rows' cotangents need a plant table)");
    if (misaligned16(g_plant_rows)) return bad(GPD_EINVAL, "g_plant_rows must be 16-byte aligned");
    return vjp_impl(bad, params, cfg, ld, num_steps, actions, action_step_stride, target_pos, plant_rows, tape, g_obs12, obs_step_stride,
                    g_reward, env_step_stride, g_kin, g_actions, g_plant_rows, stream);
}

int gpd_plant_derive_vjp(const GpdParams* nominal, const float* scales, const float* g_rows, int32_t n, int64_t ld, float* g_scales,
                         void* stream) {
    const Refuse bad{"gpd_plant_derive_vjp"};
    if (!nominal || !scales || !g_rows || !g_scales) return bad(GPD_EINVAL, "NULL nominal/scales/g_rows/g_scales");
    if (n <= 0) return bad(GPD_EINVAL, "n must be > 0");
    if (ld <= 0 || ld > 0xffffffffLL) return bad(GPD_EINVAL, "ld must be in 1 .. 2^32 - 1 (floats)");
    if (int rc = check_extent(bad, n, ld, "ld")) return rc;
    hipLaunchKernelGGL(gpd_plant_derive_vjp_kernel, dim3(blocks_for(n, 256)), dim3(256), 0, static_cast<hipStream_t>(stream), *nominal, scales,
                       g_rows, static_cast<uint32_t>(n), ld, g_scales);
    return launched(bad.who);
}

}  // extern "C"
