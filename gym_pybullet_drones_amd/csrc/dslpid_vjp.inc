/* dslpid_vjp.inc -- the adjoint of one call of the DSLPID controller (dslpid() of gpd_common.inc; control/DSLPIDControl.py:82-259) as
 * the kernels execute it: (position, velocity, rotation matrix, cached Euler angles, the targets, the nine members, the 18 gains)
 * -> (the four RPMs, the nine members after the call).  gpd_dslpid_vjp() re-runs the forward from the same inputs WITH THE SAME
 * EXPRESSIONS (every select below tests the value the forward tested) and pushes the cotangents of the outputs back to the inputs.
 * A select differentiates the branch taken and passes the cotangent where torch.clamp passes it (lo <= x <= hi); the square root of
 * `along` has its derivative selected to 0 at along <= 0 (no inf * 0).  Named scalars throughout: a runtime-indexed array would live in
 * scratch memory.  fp32.
 * Plain C, on purpose, like plant_derive_vjp.inc: the sweep in diff_pid_kernels.inc and the host program tests/c/diff_pid_host.c compile
 * THIS text, so the formulas a machine without a GPU holds against float64 autograd are the ones the device runs.  Included after gpd.h. */
#ifndef GPD_DSLPID_VJP_INC
#define GPD_DSLPID_VJP_INC

#ifndef GPD_HOST_DEVICE
#if defined(__HIPCC__) || defined(__CUDACC__)
#define GPD_HOST_DEVICE __host__ __device__
#else
#include <math.h>
#define GPD_HOST_DEVICE
#pragma clang fp contract(off)      /* as the device build (-ffp-contract=off) */
#endif
#endif

/* the hardware's 1-ulp square root and reciprocal square root on the device (fast_sqrt / fast_rsq of gpd_common.inc), libm on a host */
#if defined(__HIP_DEVICE_COMPILE__) && __HIP_DEVICE_COMPILE__
#define GPD_FAST_SQRT(x) __builtin_amdgcn_sqrtf(x)
#define GPD_FAST_RSQ(x) __builtin_amdgcn_rsqf(x)
#else
#define GPD_FAST_SQRT(x) sqrtf(x)
#define GPD_FAST_RSQ(x) (1.0f / sqrtf(x))
#endif

/* what one call of the controller reads besides the gains -- and, as a second object of the same type, the cotangents of all of it */
typedef struct GpdDslVars {
    float px, py, pz, vx, vy, vz;                        /* position, velocity */
    float r00, r01, r02, r10, r11, r12, r20, r21, r22;   /* R(q) */
    float roll, pitch, yaw;                              /* the cached Euler angles */
    float tx, ty, tz, tyaw, tvx, tvy, tvz;               /* target position, yaw, velocity (target rpy rates: zero, constants) */
    float ipx, ipy, ipz, lr, lp, ly, irx, iry, irz;      /* the members BEFORE the call: integral position error, last rpy, integral rpy error */
} GpdDslVars;

/* cotangents of the outputs: the four RPMs and the members AFTER the call */
typedef struct GpdDslOutCot {
    float rpm0, rpm1, rpm2, rpm3;
    float ipx, ipy, ipz, lr, lp, ly, irx, iry, irz;
} GpdDslOutCot;

/* cotangents of the gains, in the order p_for, i_for, d_for, p_tor, i_tor, d_tor (x, y, z each): += */
typedef struct GpdDslGainCot {
    float pf0, pf1, pf2, if0, if1, if2, df0, df1, df2, pt0, pt1, pt2, it0, it1, it2, dt0, dt1, dt2;
} GpdDslGainCot;

GPD_HOST_DEVICE static inline float gpd_dsl_clamp(float v, float lo, float hi) { return fminf(fmaxf(v, lo), hi); }
/* where torch.clamp passes the gradient */
GPD_HOST_DEVICE static inline float gpd_dsl_pass(float a, float v, float lo, float hi) { return (v >= lo && v <= hi) ? a : 0.0f; }

/* X: the inputs;  o: cotangents of the outputs;  a: receives (=) the cotangents of the inputs;  G: NULL, or += the gains' cotangents.
 * What `a` receives does not depend on G. */
GPD_HOST_DEVICE static inline __attribute__((always_inline)) void gpd_dslpid_vjp(const GpdParams* P, float dt, float inv_dt, const GpdDslVars* X, const GpdDslOutCot* o,
                                                  GpdDslVars* a, GpdDslGainCot* G) {
    /* ---- forward, dslpid()'s expressions ---- */
    const float epx = X->tx - X->px, epy = X->ty - X->py, epz = X->tz - X->pz;
    const float evx = X->tvx - X->vx, evy = X->tvy - X->vy, evz = X->tvz - X->vz;
    const float ux = fmaf(epx, dt, X->ipx), uy = fmaf(epy, dt, X->ipy), uz = fmaf(epz, dt, X->ipz);
    const float ipx = gpd_dsl_clamp(ux, -2.0f, 2.0f), ipy = gpd_dsl_clamp(uy, -2.0f, 2.0f);
    const float uz2 = gpd_dsl_clamp(uz, -2.0f, 2.0f);
    const float ipz = gpd_dsl_clamp(uz2, -0.15f, 0.15f);
    const float fx = fmaf(P->d_for[0], evx, fmaf(P->i_for[0], ipx, P->p_for[0] * epx));
    const float fy = fmaf(P->d_for[1], evy, fmaf(P->i_for[1], ipy, P->p_for[1] * epy));
    const float fz = fmaf(P->d_for[2], evz, fmaf(P->i_for[2], ipz, P->p_for[2] * epz)) + P->pid_gravity;
    const float dot = fmaf(fz, X->r22, fmaf(fy, X->r12, fx * X->r02));
    const float along = fmaxf(0.0f, dot);
    const float sq = GPD_FAST_SQRT(along * P->pid_inv_4kf);
    const float base_pwm = (sq - P->pwm2rpm_const) * P->inv_pwm2rpm_scale;
    const float fn = GPD_FAST_RSQ(fmaf(fz, fz, fmaf(fy, fy, fx * fx)));
    const float zbx = fx * fn, zby = fy * fn, zbz = fz * fn;
    float sy, cy;
    sincosf(X->tyaw, &sy, &cy);
    const float rbx = -(zbz * sy), rby = zbz * cy, rbz = fmaf(zbx, sy, -(zby * cy));
    const float yn = GPD_FAST_RSQ(fmaf(rbz, rbz, fmaf(rby, rby, rbx * rbx)));
    const float ybx = rbx * yn, yby = rby * yn, ybz = rbz * yn;
    const float xbx = fmaf(yby, zbz, -(ybz * zby)), xby = fmaf(ybz, zbx, -(ybx * zbz)), xbz = fmaf(ybx, zby, -(yby * zbx));
    const float m21 = fmaf(zbz, X->r21, fmaf(zby, X->r11, zbx * X->r01)), m12 = fmaf(ybz, X->r22, fmaf(yby, X->r12, ybx * X->r02));
    const float m02 = fmaf(xbz, X->r22, fmaf(xby, X->r12, xbx * X->r02)), m20 = fmaf(zbz, X->r20, fmaf(zby, X->r10, zbx * X->r00));
    const float m10 = fmaf(ybz, X->r20, fmaf(yby, X->r10, ybx * X->r00)), m01 = fmaf(xbz, X->r21, fmaf(xby, X->r11, xbx * X->r01));
    const float erx = m21 - m12, ery = m02 - m20, erz = m10 - m01;
    const float ewx = fmaf(-(X->roll - X->lr), inv_dt, 0.0f), ewy = fmaf(-(X->pitch - X->lp), inv_dt, 0.0f), ewz = fmaf(-(X->yaw - X->ly), inv_dt, 0.0f);
    const float wx = fmaf(-erx, dt, X->irx), wy = fmaf(-ery, dt, X->iry), wz = fmaf(-erz, dt, X->irz);
    const float wx2 = gpd_dsl_clamp(wx, -1500.0f, 1500.0f), wy2 = gpd_dsl_clamp(wy, -1500.0f, 1500.0f);
    const float irx = gpd_dsl_clamp(wx2, -1.0f, 1.0f), iry = gpd_dsl_clamp(wy2, -1.0f, 1.0f), irz = gpd_dsl_clamp(wz, -1500.0f, 1500.0f);
    const float q0 = fmaf(P->i_tor[0], irx, fmaf(P->d_tor[0], ewx, -(P->p_tor[0] * erx)));
    const float q1 = fmaf(P->i_tor[1], iry, fmaf(P->d_tor[1], ewy, -(P->p_tor[1] * ery)));
    const float q2 = fmaf(P->i_tor[2], irz, fmaf(P->d_tor[2], ewz, -(P->p_tor[2] * erz)));
    const float t0 = gpd_dsl_clamp(q0, -3200.0f, 3200.0f), t1 = gpd_dsl_clamp(q1, -3200.0f, 3200.0f), t2 = gpd_dsl_clamp(q2, -3200.0f, 3200.0f);
    const float w0 = fmaf(P->mixer[2], t2, fmaf(P->mixer[1], t1, fmaf(P->mixer[0], t0, base_pwm)));
    const float w1 = fmaf(P->mixer[5], t2, fmaf(P->mixer[4], t1, fmaf(P->mixer[3], t0, base_pwm)));
    const float w2 = fmaf(P->mixer[8], t2, fmaf(P->mixer[7], t1, fmaf(P->mixer[6], t0, base_pwm)));
    const float w3 = fmaf(P->mixer[11], t2, fmaf(P->mixer[10], t1, fmaf(P->mixer[9], t0, base_pwm)));

    /* ---- reverse ---- */
    /* rpm = scale clamp(pwm) + const;  pwm = base + mixer (t0, t1, t2) */
    const float ap0 = gpd_dsl_pass(P->pwm2rpm_scale * o->rpm0, w0, P->min_pwm, P->max_pwm);
    const float ap1 = gpd_dsl_pass(P->pwm2rpm_scale * o->rpm1, w1, P->min_pwm, P->max_pwm);
    const float ap2 = gpd_dsl_pass(P->pwm2rpm_scale * o->rpm2, w2, P->min_pwm, P->max_pwm);
    const float ap3 = gpd_dsl_pass(P->pwm2rpm_scale * o->rpm3, w3, P->min_pwm, P->max_pwm);
    const float a_base = ((ap0 + ap1) + ap2) + ap3;
    const float a_t0 = fmaf(P->mixer[9], ap3, fmaf(P->mixer[6], ap2, fmaf(P->mixer[3], ap1, P->mixer[0] * ap0)));
    const float a_t1 = fmaf(P->mixer[10], ap3, fmaf(P->mixer[7], ap2, fmaf(P->mixer[4], ap1, P->mixer[1] * ap0)));
    const float a_t2 = fmaf(P->mixer[11], ap3, fmaf(P->mixer[8], ap2, fmaf(P->mixer[5], ap1, P->mixer[2] * ap0)));
    /* the +-3200 clamps;  q_i = i_tor ir_i + d_tor ew_i - p_tor er_i */
    const float a_q0 = gpd_dsl_pass(a_t0, q0, -3200.0f, 3200.0f), a_q1 = gpd_dsl_pass(a_t1, q1, -3200.0f, 3200.0f);
    const float a_q2 = gpd_dsl_pass(a_t2, q2, -3200.0f, 3200.0f);
    if (G) {
        G->it0 = fmaf(a_q0, irx, G->it0); G->it1 = fmaf(a_q1, iry, G->it1); G->it2 = fmaf(a_q2, irz, G->it2);
        G->dt0 = fmaf(a_q0, ewx, G->dt0); G->dt1 = fmaf(a_q1, ewy, G->dt1); G->dt2 = fmaf(a_q2, ewz, G->dt2);
        G->pt0 = fmaf(-a_q0, erx, G->pt0); G->pt1 = fmaf(-a_q1, ery, G->pt1); G->pt2 = fmaf(-a_q2, erz, G->pt2);
    }
    /* the rate integrators: ir' = clamp(clamp(ir - er dt, +-1500), +-1) (z: +-1500 only) */
    const float a_ir0 = fmaf(P->i_tor[0], a_q0, o->irx), a_ir1 = fmaf(P->i_tor[1], a_q1, o->iry), a_ir2 = fmaf(P->i_tor[2], a_q2, o->irz);
    const float a_wx = gpd_dsl_pass(gpd_dsl_pass(a_ir0, wx2, -1.0f, 1.0f), wx, -1500.0f, 1500.0f);
    const float a_wy = gpd_dsl_pass(gpd_dsl_pass(a_ir1, wy2, -1.0f, 1.0f), wy, -1500.0f, 1500.0f);
    const float a_wz = gpd_dsl_pass(a_ir2, wz, -1500.0f, 1500.0f);
    a->irx = a_wx; a->iry = a_wy; a->irz = a_wz;
    const float a_erx = -fmaf(P->p_tor[0], a_q0, dt * a_wx), a_ery = -fmaf(P->p_tor[1], a_q1, dt * a_wy), a_erz = -fmaf(P->p_tor[2], a_q2, dt * a_wz);
    /* the Euler-angle finite difference ew = -(rpy - last rpy) / dt, and last rpy' = rpy */
    const float a_ewx = P->d_tor[0] * a_q0, a_ewy = P->d_tor[1] * a_q1, a_ewz = P->d_tor[2] * a_q2;
    a->lr = inv_dt * a_ewx; a->lp = inv_dt * a_ewy; a->ly = inv_dt * a_ewz;
    a->roll = fmaf(-inv_dt, a_ewx, o->lr); a->pitch = fmaf(-inv_dt, a_ewy, o->lp); a->yaw = fmaf(-inv_dt, a_ewz, o->ly);
    /* e_R = (m21 - m12, m02 - m20, m10 - m01), m_ij = col_i(R*) . col_j(R), R* = [xb yb zb] */
    float a_xbx = fmaf(a_ery, X->r02, -(a_erz * X->r01)), a_xby = fmaf(a_ery, X->r12, -(a_erz * X->r11)), a_xbz = fmaf(a_ery, X->r22, -(a_erz * X->r21));
    float a_ybx = fmaf(a_erz, X->r00, -(a_erx * X->r02)), a_yby = fmaf(a_erz, X->r10, -(a_erx * X->r12)), a_ybz = fmaf(a_erz, X->r20, -(a_erx * X->r22));
    float a_zbx = fmaf(a_erx, X->r01, -(a_ery * X->r00)), a_zby = fmaf(a_erx, X->r11, -(a_ery * X->r10)), a_zbz = fmaf(a_erx, X->r21, -(a_ery * X->r20));
    a->r00 = fmaf(a_erz, ybx, -(a_ery * zbx)); a->r10 = fmaf(a_erz, yby, -(a_ery * zby)); a->r20 = fmaf(a_erz, ybz, -(a_ery * zbz));
    a->r01 = fmaf(a_erx, zbx, -(a_erz * xbx)); a->r11 = fmaf(a_erx, zby, -(a_erz * xby)); a->r21 = fmaf(a_erx, zbz, -(a_erz * xbz));
    float a_r02 = fmaf(a_ery, xbx, -(a_erx * ybx)), a_r12 = fmaf(a_ery, xby, -(a_erx * yby)), a_r22 = fmaf(a_ery, xbz, -(a_erx * ybz));
    /* xb = yb x zb:  a_yb += zb x a_xb,  a_zb += a_xb x yb */
    a_ybx += fmaf(zby, a_xbz, -(zbz * a_xby)); a_yby += fmaf(zbz, a_xbx, -(zbx * a_xbz)); a_ybz += fmaf(zbx, a_xby, -(zby * a_xbx));
    a_zbx += fmaf(a_xby, ybz, -(a_xbz * yby)); a_zby += fmaf(a_xbz, ybx, -(a_xbx * ybz)); a_zbz += fmaf(a_xbx, yby, -(a_xby * ybx));
    /* yb = rb / |rb|,  rb = zb x (cos tyaw, sin tyaw, 0) = (-zbz sy, zbz cy, zbx sy - zby cy) */
    const float yd = fmaf(ybz, a_ybz, fmaf(yby, a_yby, ybx * a_ybx));
    const float a_rbx = yn * fmaf(-ybx, yd, a_ybx), a_rby = yn * fmaf(-yby, yd, a_yby), a_rbz = yn * fmaf(-ybz, yd, a_ybz);
    a_zbz += fmaf(cy, a_rby, -(sy * a_rbx)); a_zbx = fmaf(sy, a_rbz, a_zbx); a_zby = fmaf(-cy, a_rbz, a_zby);
    const float a_sy = fmaf(zbx, a_rbz, -(zbz * a_rbx)), a_cy = fmaf(zbz, a_rby, -(zby * a_rbz));
    a->tyaw = fmaf(a_sy, cy, -(a_cy * sy));
    /* zb = f / |f| */
    const float zd = fmaf(zbz, a_zbz, fmaf(zby, a_zby, zbx * a_zbx));
    float a_fx = fn * fmaf(-zbx, zd, a_zbx), a_fy = fn * fmaf(-zby, zd, a_zby), a_fz = fn * fmaf(-zbz, zd, a_zbz);
    /* base_pwm = (sqrt(along / 4kf) - const) / scale,  along = max(0, f . R[:, 2]): nothing passes at along <= 0 */
    const float a_sq = P->inv_pwm2rpm_scale * a_base;
    const float a_dot = dot > 0.0f ? (0.5f * P->pid_inv_4kf) * (a_sq * GPD_FAST_RSQ(along * P->pid_inv_4kf)) : 0.0f;
    a_fx = fmaf(a_dot, X->r02, a_fx); a_fy = fmaf(a_dot, X->r12, a_fy); a_fz = fmaf(a_dot, X->r22, a_fz);
    a->r02 = fmaf(a_dot, fx, a_r02); a->r12 = fmaf(a_dot, fy, a_r12); a->r22 = fmaf(a_dot, fz, a_r22);
    /* f_i = d_for ev_i + i_for ip'_i + p_for ep_i (+ gravity) */
    if (G) {
        G->df0 = fmaf(a_fx, evx, G->df0); G->df1 = fmaf(a_fy, evy, G->df1); G->df2 = fmaf(a_fz, evz, G->df2);
        G->if0 = fmaf(a_fx, ipx, G->if0); G->if1 = fmaf(a_fy, ipy, G->if1); G->if2 = fmaf(a_fz, ipz, G->if2);
        G->pf0 = fmaf(a_fx, epx, G->pf0); G->pf1 = fmaf(a_fy, epy, G->pf1); G->pf2 = fmaf(a_fz, epz, G->pf2);
    }
    const float a_evx = P->d_for[0] * a_fx, a_evy = P->d_for[1] * a_fy, a_evz = P->d_for[2] * a_fz;
    /* the position integrators: ip' = clamp(ip + ep dt, +-2), z nested in +-0.15 */
    const float a_ux = gpd_dsl_pass(fmaf(P->i_for[0], a_fx, o->ipx), ux, -2.0f, 2.0f);
    const float a_uy = gpd_dsl_pass(fmaf(P->i_for[1], a_fy, o->ipy), uy, -2.0f, 2.0f);
    const float a_uz = gpd_dsl_pass(gpd_dsl_pass(fmaf(P->i_for[2], a_fz, o->ipz), uz2, -0.15f, 0.15f), uz, -2.0f, 2.0f);
    a->ipx = a_ux; a->ipy = a_uy; a->ipz = a_uz;
    const float a_epx = fmaf(dt, a_ux, P->p_for[0] * a_fx), a_epy = fmaf(dt, a_uy, P->p_for[1] * a_fy), a_epz = fmaf(dt, a_uz, P->p_for[2] * a_fz);
    /* the errors: ep = t - p, ev = tv - v */
    a->tx = a_epx; a->ty = a_epy; a->tz = a_epz; a->px = -a_epx; a->py = -a_epy; a->pz = -a_epz;
    a->tvx = a_evx; a->tvy = a_evy; a->tvz = a_evz; a->vx = -a_evx; a->vy = -a_evy; a->vz = -a_evz;
}

#endif
