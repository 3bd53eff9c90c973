/* ctbr_math.inc -- the arithmetic of the thrust-and-body-rate controller (include/gpd.h: gpd_ctbr, gpd_rollout_ctbr), stated once.
 *   (a) gpd_ctbr_outer      the reference's CTBRControl.computeControl (control/CTBRControl.py:149-168): position and velocity errors ->
 *                           a mass-normalised thrust [m/s^2] and three body rates [rad/s]
 *   (b) gpd_ctbr_rate_loop  the stand-in for the flight controller the reference leaves to Betaflight (envs/BetaAviary.py): clipped
 *                           command + the integrator's body rates -> four RPMs, evaluated every physics sub-step.  No integrator, no
 *                           derivative term, no state.  The reference has no such code.
 * Plain C, on purpose, like mppi_math.inc: the kernels in ctbr.inc and the host program tests/c/ctbr_host.c compile THIS text.  fp32,
 * contraction off, every fused multiply-add an explicit fmaf in one fixed order.  The device takes sqrt, 1/sqrt and 1/x from the
 * 1-ulp hardware instructions (as the physics does, gpd_common.inc), the host from libm.  Included after gpd.h. */
#ifndef GPD_CTBR_MATH_INC
#define GPD_CTBR_MATH_INC

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

#if defined(__HIP_DEVICE_COMPILE__)
#define GPD_CTBR_SQRT(x) __builtin_amdgcn_sqrtf(x)
#define GPD_CTBR_RSQ(x) __builtin_amdgcn_rsqf(x)
#else
#define GPD_CTBR_SQRT(x) sqrtf(x)
#define GPD_CTBR_RSQ(x) (1.0f / sqrtf(x))
#endif

GPD_HOST_DEVICE static inline float gpd_ctbr_clip(float v, float lo, float hi) { return fminf(fmaxf(v, lo), hi); }

/* (a) The outer loop.  q = (qx, qy, qz, qw) is the state's order; the target velocity of a call without one is zero.
 *   tar_acc = K_P (target_pos - pos) + K_D (target_vel - vel) - G,  G = (0, 0, -g)                                         (:153-155)
 *   thrust  = tar_acc . (q z q*)           (third column of the rotation, NOT normalised by |q|^2: transforms3d's rotate_vector) (:156)
 *   z_b = unit(tar_acc), x_b = unit(y^ x z_b), y_b = unit(z_b x x_b); q_t = the quaternion of [x_b y_b z_b]               (:158-161)
 *   q_e = conj(q) (x) q_t; rates = 2 K_RATES q_e.xyz, negated when q_e.w < 0                                               (:163-166)
 * The last negation makes the rates independent of the sign the matrix -> quaternion step picks, so Shepperd's four cases are
 * selects here (the reference's route, an eigenvector with w >= 0, returns the same rotation). */
GPD_HOST_DEVICE static inline void gpd_ctbr_outer(const GpdCtbr* c, float px, float py, float pz, float qx, float qy, float qz, float qw,
                                                  float vx, float vy, float vz, float tx, float ty, float tz, float tvx, float tvy, float tvz,
                                                  float cmd[4]) {
    const float ax = fmaf(c->k_d[0], tvx - vx, c->k_p[0] * (tx - px));
    const float ay = fmaf(c->k_d[1], tvy - vy, c->k_p[1] * (ty - py));
    const float az = fmaf(c->k_d[2], tvz - vz, c->k_p[2] * (tz - pz)) + c->g;
    /* q (0, 0, 1) q* */
    const float rzx = 2.0f * fmaf(qx, qz, qw * qy), rzy = 2.0f * fmaf(qy, qz, -(qw * qx));
    const float rzz = fmaf(qw, qw, qz * qz) - fmaf(qx, qx, qy * qy);
    cmd[0] = fmaf(az, rzz, fmaf(ay, rzy, ax * rzx));
    /* the target frame */
    const float an = GPD_CTBR_RSQ(fmaf(az, az, fmaf(ay, ay, ax * ax)));
    const float zx = ax * an, zy = ay * an, zz = az * an;
    const float xn = GPD_CTBR_RSQ(fmaf(zx, zx, zz * zz));                  /* y^ x z_b = (zz, 0, -zx) */
    const float xx = zz * xn, xz = -(zx * xn);
    float yx = zy * xz, yy = fmaf(zz, xx, -(zx * xz)), yz = -(zy * xx);    /* z_b x x_b, x_b.y = 0 */
    const float yn = GPD_CTBR_RSQ(fmaf(yz, yz, fmaf(yy, yy, yx * yx)));
    yx *= yn; yy *= yn; yz *= yn;
    /* M = [x_b y_b z_b] (columns): m00 = xx, m10 = 0, m20 = xz; m01 = yx, m11 = yy, m21 = yz; m02 = zx, m12 = zy, m22 = zz */
    const float tr = (xx + yy) + zz;
    const int c0 = tr > 0.0f, c1 = !c0 && xx > yy && xx > zz, c2 = !c0 && !c1 && yy > zz;
    const float d = 1.0f + (c0 ? tr : c1 ? (xx - yy) - zz : c2 ? (yy - xx) - zz : (zz - xx) - yy);
    const float r = 0.5f * GPD_CTBR_RSQ(d), big = d * r;
    const float a = (yz - zy) * r, b = (zx - xz) * r, e = -(yx * r);       /* (m21 - m12), (m02 - m20), (m10 - m01) over 2 sqrt(d) */
    const float p = yx * r, q = (zx + xz) * r, s = (zy + yz) * r;          /* (m01 + m10), (m02 + m20), (m12 + m21) */
    const float tw = c0 ? big : c1 ? a : c2 ? b : e;
    const float tqx = c0 ? a : c1 ? big : c2 ? p : q;
    const float tqy = c0 ? b : c1 ? p : c2 ? big : s;
    const float tqz = c0 ? e : c1 ? q : c2 ? s : big;
    /* conj(q) (x) q_t */
    const float ew = fmaf(qz, tqz, fmaf(qy, tqy, fmaf(qx, tqx, qw * tw)));
    const float ex = fmaf(qz, tqy, fmaf(-qy, tqz, fmaf(-qx, tw, qw * tqx)));
    const float ey = fmaf(-qz, tqx, fmaf(qx, tqz, fmaf(-qy, tw, qw * tqy)));
    const float ez = fmaf(qy, tqx, fmaf(-qx, tqy, fmaf(-qz, tw, qw * tqz)));
    const float sg = ew < 0.0f ? -2.0f : 2.0f;
    cmd[1] = (sg * c->k_rates[0]) * ex;
    cmd[2] = (sg * c->k_rates[1]) * ey;
    cmd[3] = (sg * c->k_rates[2]) * ez;
}

/* (b) The rate loop, once per physics sub-step; (wx, wy, wz): the body rates the integrator carries; M, J: the NOMINAL airframe.
 *   1. thrust to [0, thrust_max], each rate to +-rate_max (BetaAviary.ctbr2beta's limits, envs/BetaAviary.py:176-188)
 *   2. tau = J (k_rate (w_cmd - w)) + w x (J w)
 *   3. T = M thrust
 *   4. f_i = T/4 + alloc[i] . tau: the exact inverse of the integrator's torque rows, host-computed in float64
 *   5. rpm_i = sqrt(clip(f_i, 0, f_max) / KF)
 * A NaN command leaves the clips as their bounds' side (fminf / fmaxf), like the DSLPID path's clips. */
GPD_HOST_DEVICE static inline void gpd_ctbr_rate_loop(const GpdCtbr* c, float M, float Jx, float Jy, float Jz, const float cmd[4], float wx,
                                                      float wy, float wz, float rpm[4]) {
    const float thr = gpd_ctbr_clip(cmd[0], 0.0f, c->thrust_max);
    const float cx = gpd_ctbr_clip(cmd[1], -c->rate_max, c->rate_max), cy = gpd_ctbr_clip(cmd[2], -c->rate_max, c->rate_max),
                cz = gpd_ctbr_clip(cmd[3], -c->rate_max, c->rate_max);
    const float jwx = Jx * wx, jwy = Jy * wy, jwz = Jz * wz;
    const float taux = fmaf(Jx, c->k_rate[0] * (cx - wx), fmaf(wy, jwz, -(wz * jwy)));
    const float tauy = fmaf(Jy, c->k_rate[1] * (cy - wy), fmaf(wz, jwx, -(wx * jwz)));
    const float tauz = fmaf(Jz, c->k_rate[2] * (cz - wz), fmaf(wx, jwy, -(wy * jwx)));
    const float t4 = 0.25f * (M * thr);
#if defined(__HIPCC__) || defined(__CUDACC__)
#pragma unroll
#endif
    for (int i = 0; i < 4; ++i) {
        const float f = fmaf(c->alloc[3 * i + 2], tauz, fmaf(c->alloc[3 * i + 1], tauy, fmaf(c->alloc[3 * i], taux, t4)));
        rpm[i] = GPD_CTBR_SQRT(gpd_ctbr_clip(f, 0.0f, c->f_max) * c->inv_kf);
    }
}

#endif
