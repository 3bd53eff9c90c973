/* ctbr_vjp.inc -- the adjoints of the two loops of ctbr_math.inc (include/gpd.h: gpd_rollout_vjp_ctbr), stated once.
 *   (a) gpd_ctbr_rate_loop_vjp   cotangents of the four rotor thrust deviations (what substep_vjp hands back) -> the command, the body
 *                                rates, the rate gains
 *   (b) gpd_ctbr_outer_vjp       cotangent of the command -> position, quaternion, velocity, target position, target velocity, the
 *                                outer loop's gains
 * Plain C, like dslpid_vjp.inc: the kernels of diff_ctbr_kernels.inc and the host program tests/c/diff_ctbr_host.c compile THIS text.
 * fp32, contraction off, explicit fmaf.  The adjoint is that of the function AS EXECUTED: a clip passes its cotangent on lo <= x <= hi and
 * exactly nothing outside, Shepperd's four cases and the q_e.w < 0 negation differentiate the branch taken.  Both sides of every select
 * are evaluated and one is chosen (a branch that writes through a pointer sends the caller's cotangents to scratch memory, DESIGN.md
 * section 3.12).  Included after ctbr_math.inc. */
#ifndef GPD_CTBR_VJP_INC
#define GPD_CTBR_VJP_INC

GPD_HOST_DEVICE static inline float gpd_ctbr_pass(float v, float lo, float hi, float g) { return (v >= lo && v <= hi) ? g : 0.0f; }

/* (a) Adjoint of  (cmd, w) -> g[4],  g_i = thrust_dev(rpm_i),  rpm = gpd_ctbr_rate_loop(cmd, w).
 * The chain f -> rpm = sqrt(clip(f) inv_kf) -> g = KF_plant rpm^2 + const is ONE map: dg_i/df_i = kf_plant * inv_kf inside the rotor clip
 * and 0 outside; nothing is divided by an rpm (a rotor held at 0 would give 0 * inf).
 *   kf_plant   the KF the PHYSICS uses (GpdParams.KF, or the drone's plant row); c->inv_kf is the controller's nominal 1/KF
 *   ag[4]      cotangents of the thrust deviations
 *   acmd[4] += cotangent of the command;  aw[3] += cotangent of the body rates;  akr: NULL, or [3] += cotangent of k_rate */
GPD_HOST_DEVICE static inline void gpd_ctbr_rate_loop_vjp(const GpdCtbr* c, float M, float Jx, float Jy, float Jz, float kf_plant,
                                                          const float cmd[4], float wx, float wy, float wz, const float ag[4],
                                                          float acmd[4], float aw[3], float* akr) {
    /* ---- forward: what the reverse pass needs of it (the expressions of gpd_ctbr_rate_loop) */
    const float thr = gpd_ctbr_clip(cmd[0], 0.0f, c->thrust_max);
    const float cx = gpd_ctbr_clip(cmd[1], -c->rate_max, c->rate_max), cy = gpd_ctbr_clip(cmd[2], -c->rate_max, c->rate_max),
                cz = gpd_ctbr_clip(cmd[3], -c->rate_max, c->rate_max);
    const float jwx = Jx * wx, jwy = Jy * wy, jwz = Jz * wz;
    const float taux = fmaf(Jx, c->k_rate[0] * (cx - wx), fmaf(wy, jwz, -(wz * jwy)));
    const float tauy = fmaf(Jy, c->k_rate[1] * (cy - wy), fmaf(wz, jwx, -(wx * jwz)));
    const float tauz = fmaf(Jz, c->k_rate[2] * (cz - wz), fmaf(wx, jwy, -(wy * jwx)));
    const float t4 = 0.25f * (M * thr);
    const float dgdf = kf_plant * c->inv_kf;
    /* ---- reverse: the rotors, f_i = t4 + alloc[i] . tau */
    float a_t4 = 0.0f, a_tx = 0.0f, a_ty = 0.0f, a_tz = 0.0f;
#if defined(__HIPCC__) || defined(__CUDACC__)
#pragma unroll
#endif
    for (int i = 0; i < 4; ++i) {
        const float f = fmaf(c->alloc[3 * i + 2], tauz, fmaf(c->alloc[3 * i + 1], tauy, fmaf(c->alloc[3 * i], taux, t4)));
        const float af = gpd_ctbr_pass(f, 0.0f, c->f_max, ag[i] * dgdf);
        a_t4 += af;
        a_tx = fmaf(c->alloc[3 * i], af, a_tx);
        a_ty = fmaf(c->alloc[3 * i + 1], af, a_ty);
        a_tz = fmaf(c->alloc[3 * i + 2], af, a_tz);
    }
    /* tau = J k_rate (w_cmd - w) + w x (J w) */
    const float px = Jx * c->k_rate[0] * a_tx, py = Jy * c->k_rate[1] * a_ty, pz = Jz * c->k_rate[2] * a_tz;
    acmd[0] += gpd_ctbr_pass(cmd[0], 0.0f, c->thrust_max, 0.25f * M * a_t4);
    acmd[1] += gpd_ctbr_pass(cmd[1], -c->rate_max, c->rate_max, px);
    acmd[2] += gpd_ctbr_pass(cmd[2], -c->rate_max, c->rate_max, py);
    acmd[3] += gpd_ctbr_pass(cmd[3], -c->rate_max, c->rate_max, pz);
    /* (w x J w)_x = wy wz (Jz - Jy), _y = wz wx (Jx - Jz), _z = wx wy (Jy - Jx): the transpose of its Jacobian */
    const float jzy = Jz - Jy, jxz = Jx - Jz, jyx = Jy - Jx;
    aw[0] += fmaf(a_ty, wz * jxz, a_tz * (wy * jyx)) - px;
    aw[1] += fmaf(a_tx, wz * jzy, a_tz * (wx * jyx)) - py;
    aw[2] += fmaf(a_tx, wy * jzy, a_ty * (wx * jxz)) - pz;
    if (akr) {
        akr[0] = fmaf(Jx * (cx - wx), a_tx, akr[0]);
        akr[1] = fmaf(Jy * (cy - wy), a_ty, akr[1]);
        akr[2] = fmaf(Jz * (cz - wz), a_tz, akr[2]);
    }
}

/* (b) Adjoint of gpd_ctbr_outer at the same arguments.  ac[4]: the command's cotangent.  Written (not added to): gp[3] position,
 * gq[4] quaternion x y z w, gv[3] velocity, gt[3] target position, gtv[3] target velocity.  agn: NULL, or [9] += the cotangents of
 * k_p[3] | k_d[3] | k_rates[3].  The three rsq normalisations are differentiated as 1/sqrt: for u = v / |v|, the cotangent of v is
 * (a_u - u (u . a_u)) / |v|. */
GPD_HOST_DEVICE static inline void gpd_ctbr_outer_vjp(const GpdCtbr* c, float px, float py, float pz, float qx, float qy, float qz, float qw,
                                                      float vx, float vy, float vz, float tx, float ty, float tz, float tvx, float tvy,
                                                      float tvz, const float ac[4], float gp[3], float gq[4], float gv[3], float gt[3],
                                                      float gtv[3], float* agn) {
    /* ---- forward (the expressions of gpd_ctbr_outer) */
    const float ax = fmaf(c->k_d[0], tvx - vx, c->k_p[0] * (tx - px));
    const float ay = fmaf(c->k_d[1], tvy - vy, c->k_p[1] * (ty - py));
    const float az = fmaf(c->k_d[2], tvz - vz, c->k_p[2] * (tz - pz)) + c->g;
    const float rzx = 2.0f * fmaf(qx, qz, qw * qy), rzy = 2.0f * fmaf(qy, qz, -(qw * qx));
    const float rzz = fmaf(qw, qw, qz * qz) - fmaf(qx, qx, qy * qy);
    const float an = GPD_CTBR_RSQ(fmaf(az, az, fmaf(ay, ay, ax * ax)));
    const float zx = ax * an, zy = ay * an, zz = az * an;
    const float xn = GPD_CTBR_RSQ(fmaf(zx, zx, zz * zz));
    const float xx = zz * xn, xz = -(zx * xn);
    float yx = zy * xz, yy = fmaf(zz, xx, -(zx * xz)), yz = -(zy * xx);
    const float yn = GPD_CTBR_RSQ(fmaf(yz, yz, fmaf(yy, yy, yx * yx)));
    yx *= yn; yy *= yn; yz *= yn;
    const float tr = (xx + yy) + zz;
    const int c0 = tr > 0.0f, c1 = !c0 && xx > yy && xx > zz, c2 = !c0 && !c1 && yy > zz, c3 = !c0 && !c1 && !c2;
    const float d = 1.0f + (c0 ? tr : c1 ? (xx - yy) - zz : c2 ? (yy - xx) - zz : (zz - xx) - yy);
    const float r = 0.5f * GPD_CTBR_RSQ(d), big = d * r;
    const float a = (yz - zy) * r, b = (zx - xz) * r, e = -(yx * r);
    const float p = yx * r, q = (zx + xz) * r, s = (zy + yz) * r;
    const float tw = c0 ? big : c1 ? a : c2 ? b : e;
    const float tqx = c0 ? a : c1 ? big : c2 ? p : q;
    const float tqy = c0 ? b : c1 ? p : c2 ? big : s;
    const float tqz = c0 ? e : c1 ? q : c2 ? s : big;
    const float ew = fmaf(qz, tqz, fmaf(qy, tqy, fmaf(qx, tqx, qw * tw)));
    const float ex = fmaf(qz, tqy, fmaf(-qy, tqz, fmaf(-qx, tw, qw * tqx)));
    const float ey = fmaf(-qz, tqx, fmaf(qx, tqz, fmaf(-qy, tw, qw * tqy)));
    const float ez = fmaf(qy, tqx, fmaf(-qx, tqy, fmaf(-qz, tw, qw * tqz)));
    const float sg = ew < 0.0f ? -2.0f : 2.0f;
    /* ---- reverse: rates = sg k_rates q_e.xyz; q_e = conj(q) (x) q_t is bilinear */
    const float a_ex = (sg * c->k_rates[0]) * ac[1], a_ey = (sg * c->k_rates[1]) * ac[2], a_ez = (sg * c->k_rates[2]) * ac[3];
    float a_qx = fmaf(a_ey, tqz, -fmaf(a_ex, tw, a_ez * tqy));
    float a_qy = fmaf(a_ez, tqx, -fmaf(a_ex, tqz, a_ey * tw));
    float a_qz = fmaf(a_ex, tqy, -fmaf(a_ey, tqx, a_ez * tw));
    float a_qw = fmaf(a_ex, tqx, fmaf(a_ey, tqy, a_ez * tqz));
    const float a_tqx = fmaf(a_ez, qy, fmaf(a_ex, qw, -(a_ey * qz)));
    const float a_tqy = fmaf(a_ey, qw, fmaf(a_ex, qz, -(a_ez * qx)));
    const float a_tqz = fmaf(a_ez, qw, fmaf(a_ey, qx, -(a_ex * qy)));
    const float a_tw = -fmaf(a_ez, qz, fmaf(a_ey, qy, a_ex * qx));
    /* Shepperd's case: which of big, a, b, e, p, q, s each component was */
    const float a_big = c0 ? a_tw : c1 ? a_tqx : c2 ? a_tqy : a_tqz;
    const float a_a = c0 ? a_tqx : c1 ? a_tw : 0.0f;
    const float a_b = c0 ? a_tqy : c2 ? a_tw : 0.0f;
    const float a_e = c0 ? a_tqz : c3 ? a_tw : 0.0f;
    const float a_p = c1 ? a_tqy : c2 ? a_tqx : 0.0f;
    const float a_q = c1 ? a_tqz : c3 ? a_tqx : 0.0f;
    const float a_s = c2 ? a_tqz : c3 ? a_tqy : 0.0f;
    /* r = 1 / (2 sqrt d): dr/dd = -2 r^3; big = d r */
    const float a_r = fmaf(a_big, d, fmaf(a_s, zy + yz, fmaf(a_q, zx + xz, fmaf(a_p - a_e, yx, fmaf(a_b, zx - xz, a_a * (yz - zy))))));
    const float a_d = fmaf(a_big, r, -2.0f * ((r * r) * r) * a_r);
    float a_yx = (a_p - a_e) * r, a_yy = (c0 || c2) ? a_d : -a_d, a_yz = (a_a + a_s) * r;
    float a_zx = (a_b + a_q) * r, a_zy = (a_s - a_a) * r, a_zz = (c0 || c3) ? a_d : -a_d;
    float a_xx = (c0 || c1) ? a_d : -a_d, a_xz = (a_q - a_b) * r;
    /* y_b = unit(y0), y0 = z_b x x_b = (zy xz, zz xx - zx xz, -zy xx) */
    const float yd = fmaf(yz, a_yz, fmaf(yy, a_yy, yx * a_yx));
    const float a_y0x = yn * fmaf(-yx, yd, a_yx), a_y0y = yn * fmaf(-yy, yd, a_yy), a_y0z = yn * fmaf(-yz, yd, a_yz);
    a_zy += fmaf(a_y0x, xz, -(a_y0z * xx));
    a_xz += fmaf(a_y0x, zy, -(a_y0y * zx));
    a_zz = fmaf(a_y0y, xx, a_zz);
    a_xx += fmaf(a_y0y, zz, -(a_y0z * zy));
    a_zx = fmaf(-a_y0y, xz, a_zx);
    /* x_b = unit(u), u = (zz, -zx) */
    const float xd = fmaf(xz, a_xz, xx * a_xx);
    a_zz = fmaf(xn, fmaf(-xx, xd, a_xx), a_zz);
    a_zx = fmaf(-xn, fmaf(-xz, xd, a_xz), a_zx);
    /* z_b = unit(tar_acc); thrust = tar_acc . (q z q*) */
    const float zd = fmaf(zz, a_zz, fmaf(zy, a_zy, zx * a_zx));
    const float a_ax = fmaf(ac[0], rzx, an * fmaf(-zx, zd, a_zx));
    const float a_ay = fmaf(ac[0], rzy, an * fmaf(-zy, zd, a_zy));
    const float a_az = fmaf(ac[0], rzz, an * fmaf(-zz, zd, a_zz));
    const float a_rzx = 2.0f * (ac[0] * ax), a_rzy = 2.0f * (ac[0] * ay), a_rzz = 2.0f * (ac[0] * az);
    a_qx += fmaf(a_rzx, qz, -fmaf(a_rzy, qw, a_rzz * qx));
    a_qy += fmaf(a_rzx, qw, fmaf(a_rzy, qz, -(a_rzz * qy)));
    a_qz += fmaf(a_rzx, qx, fmaf(a_rzy, qy, a_rzz * qz));
    a_qw += fmaf(a_rzx, qy, fmaf(a_rzz, qw, -(a_rzy * qx)));
    gq[0] = a_qx; gq[1] = a_qy; gq[2] = a_qz; gq[3] = a_qw;
    /* tar_acc = k_p (target - pos) + k_d (target_vel - vel) + (0, 0, g) */
    gt[0] = c->k_p[0] * a_ax; gt[1] = c->k_p[1] * a_ay; gt[2] = c->k_p[2] * a_az;
    gtv[0] = c->k_d[0] * a_ax; gtv[1] = c->k_d[1] * a_ay; gtv[2] = c->k_d[2] * a_az;
    gp[0] = -gt[0]; gp[1] = -gt[1]; gp[2] = -gt[2];
    gv[0] = -gtv[0]; gv[1] = -gtv[1]; gv[2] = -gtv[2];
    if (agn) {
        agn[0] = fmaf(tx - px, a_ax, agn[0]); agn[1] = fmaf(ty - py, a_ay, agn[1]); agn[2] = fmaf(tz - pz, a_az, agn[2]);
        agn[3] = fmaf(tvx - vx, a_ax, agn[3]); agn[4] = fmaf(tvy - vy, a_ay, agn[4]); agn[5] = fmaf(tvz - vz, a_az, agn[5]);
        agn[6] = fmaf(sg * ex, ac[1], agn[6]); agn[7] = fmaf(sg * ey, ac[2], agn[7]); agn[8] = fmaf(sg * ez, ac[3], agn[8]);
    }
}

#endif
