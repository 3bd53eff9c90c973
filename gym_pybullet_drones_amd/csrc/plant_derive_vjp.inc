/* plant_derive_vjp.inc -- one drone of gpd_plant_derive_vjp (include/gpd.h): the transpose of gpd_plant_derive's Jacobian at the
 * drone's scales s[GPD_NUM_SCALES], applied to the cotangents g[GPD_PLANT_ROWS] of its derived rows.  Every row is a product or a
 * quotient of a nominal field and one or two scales (include/gpd.h GPD_PLANT_*), so every line below is the derivative of one or
 * more of those rows.  float64 throughout; the caller rounds each output once.
 * Plain C, on purpose: the kernel in diff_kernels.inc and the host program tests/c/sysid_host.c compile THIS text, so the formulas a
 * machine without a GPU holds against a numerical Jacobian are the ones the device runs.  Included after gpd.h. */
#ifndef GPD_PLANT_DERIVE_VJP_INC
#define GPD_PLANT_DERIVE_VJP_INC

#if defined(__HIPCC__) || defined(__CUDACC__)
#define GPD_HOST_DEVICE __host__ __device__
#else
#define GPD_HOST_DEVICE
#endif

GPD_HOST_DEVICE static inline void gpd_plant_derive_vjp_one(const GpdParams* P, const double* s, const double* g, double* out) {
    const double m = s[GPD_SCALE_MASS], kf = s[GPD_SCALE_KF], km = s[GPD_SCALE_KM], ht = P->hover_thrust;
    int k;
    /* M = M_n m, inv_M = inv_M_n / m, GRAVITY = GRAVITY_n m, HOVER_THRUST = ht m, HOVER_RESID = resid_n kf + (kf - m) ht, NORM_GAP = (m - kf) ht */
    out[GPD_SCALE_MASS] = (double)P->M * g[GPD_PLANT_M] - (double)P->inv_M / (m * m) * g[GPD_PLANT_INV_M] + (double)P->GRAVITY * g[GPD_PLANT_GRAVITY] +
                          ht * (g[GPD_PLANT_HOVER_THRUST] - g[GPD_PLANT_HOVER_RESID] + g[GPD_PLANT_NORM_GAP]);
    /* J[k] = J_n[k] s, J_INV[k] = J_INV_n[k] / s */
#pragma unroll
    for (k = 0; k < 3; ++k) {
        const double sk = s[GPD_SCALE_IXX + k];
        out[GPD_SCALE_IXX + k] = (double)P->J[k] * g[GPD_PLANT_J + k] - (double)P->J_INV[k] / (sk * sk) * g[GPD_PLANT_J_INV + k];
    }
    /* KF = KF_n kf, KM_OVER_KF = r_n km / kf, HOVER_RESID and NORM_GAP as above, NORM_THRUST = ht kf */
    out[GPD_SCALE_KF] = (double)P->KF * g[GPD_PLANT_KF] - (double)P->km_over_kf * km / (kf * kf) * g[GPD_PLANT_KM_OVER_KF] +
                        (double)P->hover_resid * g[GPD_PLANT_HOVER_RESID] +
                        ht * (g[GPD_PLANT_HOVER_RESID] + g[GPD_PLANT_NORM_THRUST] - g[GPD_PLANT_NORM_GAP]);
    out[GPD_SCALE_KM] = (double)P->km_over_kf / kf * g[GPD_PLANT_KM_OVER_KF];
    /* DRAG[0], DRAG[1] = drag_n s_xy, DRAG[2] = drag_n s_z, GND_EFF = gnd_n s */
    out[GPD_SCALE_DRAG_XY] = (double)P->drag_coeff[0] * g[GPD_PLANT_DRAG] + (double)P->drag_coeff[1] * g[GPD_PLANT_DRAG + 1];
    out[GPD_SCALE_DRAG_Z] = (double)P->drag_coeff[2] * g[GPD_PLANT_DRAG + 2];
    out[GPD_SCALE_GND_EFF] = (double)P->gnd_eff_coeff * g[GPD_PLANT_GND_EFF];
}

#endif
