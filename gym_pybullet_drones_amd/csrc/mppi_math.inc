/* mppi_math.inc -- the arithmetic of gpd_mppi (include/gpd.h) that is not physics: the counter-based noise, the clamped perturbation,
 * the running cost of one step from the quantities the kernel has at hand, and a sample's weight.  fp32 throughout.
 * Plain C, on purpose, like obstacle_math.inc: the kernel in mppi.inc and the host program tests/c/mppi_host.c compile THIS text, so the
 * generator a machine without a GPU holds bit for bit against the numpy restatement (tests/helpers/mppi_f64.py) is the one the device
 * runs.  The reference has no such code: it has no planner.  Included after gpd.h. */
#ifndef GPD_MPPI_MATH_INC
#define GPD_MPPI_MATH_INC

#include <stdint.h>

#ifndef GPD_HOST_DEVICE
#if defined(__HIPCC__) || defined(__CUDACC__)
#define GPD_HOST_DEVICE __host__ __device__
#else
#include <math.h>
#define GPD_HOST_DEVICE
#pragma clang fp contract(off)      /* as the device build (-ffp-contract=off) */
#endif
#endif

/* Philox4x32-10 (Salmon et al., "Parallel random numbers: as easy as 1, 2, 3", SC'11): ten rounds of two 32 x 32 -> 64 multiplies,
 * the key bumped by the Weyl increments between them.  Scalars, no arrays: every word stays in a register. */
GPD_HOST_DEVICE static inline void gpd_philox4x32(uint32_t c0, uint32_t c1, uint32_t c2, uint32_t c3, uint32_t k0, uint32_t k1, uint32_t* o0,
                                                  uint32_t* o1, uint32_t* o2, uint32_t* o3) {
#if defined(__HIPCC__) || defined(__CUDACC__)
#pragma unroll
#endif
    for (int r = 0; r < 10; ++r) {
        const uint64_t p0 = (uint64_t)0xD2511F53u * c0, p1 = (uint64_t)0xCD9E8D57u * c2;
        const uint32_t n0 = (uint32_t)(p1 >> 32) ^ c1 ^ k0, n2 = (uint32_t)(p0 >> 32) ^ c3 ^ k1;
        c1 = (uint32_t)p1;
        c3 = (uint32_t)p0;
        c0 = n0;
        c2 = n2;
        k0 += 0x9E3779B9u;
        k1 += 0xBB67AE85u;
    }
    *o0 = c0; *o1 = c1; *o2 = c2; *o3 = c3;
}

/* a word -> a uniform in (0, 1]: the float32 value of ((x >> 8) + 0.5) 2^-24.  The sum is exact below 2^23 and rounds to even above
 * (25 significant bits), so the value is never 0 and is 1 for the one top word -- whose logarithm is 0, not a NaN */
GPD_HOST_DEVICE static inline float gpd_mppi_uniform(uint32_t x) { return ((float)(x >> 8) + 0.5f) * 5.9604644775390625e-8f; }

/* Box-Muller on one pair of uniforms, with the accurate logf / sincosf (not the fast builtins) */
GPD_HOST_DEVICE static inline void gpd_mppi_box_muller(float u1, float u2, float* z0, float* z1) {
    const float r = sqrtf(-2.0f * logf(u1));
    float s, c;
    sincosf(6.28318530717958647692f * u2, &s, &c);
    *z0 = r * c;
    *z1 = r * s;
}

/* the four standard normals of (drone n, sample m, step h, iteration): counter (n, m, h, iteration), key = seed; z0, z1 from words
 * 0, 1 and z2, z3 from words 2, 3 */
GPD_HOST_DEVICE static inline void gpd_mppi_normals(uint32_t n, uint32_t m, uint32_t h, uint32_t iteration, uint32_t seed0, uint32_t seed1,
                                                    float* z0, float* z1, float* z2, float* z3) {
    uint32_t x0, x1, x2, x3;
    gpd_philox4x32(n, m, h, iteration, seed0, seed1, &x0, &x1, &x2, &x3);
    gpd_mppi_box_muller(gpd_mppi_uniform(x0), gpd_mppi_uniform(x1), z0, z1);
    gpd_mppi_box_muller(gpd_mppi_uniform(x2), gpd_mppi_uniform(x3), z2, z3);
}

/* one component of a sample's action: clamp(u + sigma z, lo, hi); sigma = 0 gives clamp(u) whatever z is */
GPD_HOST_DEVICE static inline float gpd_mppi_perturb(float u, float sigma, float z, float lo, float hi) {
    return fminf(fmaxf(fmaf(sigma, z, u), lo), hi);
}

/* the running cost of one step (include/gpd.h): dp2 = |p - goal|^2, v2 = |v|^2, tilt = 1 - R22, w2 = |omega_body|^2, d the clearance
 * (+inf without a list: the hinge is then 0); w_pos already carries w_term on the last step */
GPD_HOST_DEVICE static inline float gpd_mppi_step_cost(float w_pos, float w_vel, float w_tilt, float w_rate, float w_obs, float obst_margin,
                                                       float collision_radius, float dp2, float v2, float tilt, float w2, float d) {
    const float pen = fmaxf(0.0f, obst_margin - (d - collision_radius));
    return fmaf(w_obs, pen * pen, fmaf(w_rate, w2, fmaf(w_tilt, tilt, fmaf(w_vel, v2, w_pos * dp2))));
}

/* is S a finite cost?  (false for NaN and both infinities) */
GPD_HOST_DEVICE static inline int gpd_mppi_finite(float S) { return fabsf(S) <= 3.4028234e38f; }

/* a sample's weight exp(-(S - S_min) / lambda); 0 for a cost that is not finite */
GPD_HOST_DEVICE static inline float gpd_mppi_weight(float S, float S_min, float inv_lambda) {
    return gpd_mppi_finite(S) ? expf(-(S - S_min) * inv_lambda) : 0.0f;
}

#endif
