"""What the tests of the gradients with respect to the plant scales (tests/test_host_sysid.py, tests/test_gpu_sysid.py) add to the
yardstick of tests/helpers/diff_f64.py, whose `reference_grads(..., wrt_scales=True)` takes the `[9, n]` scale factors (include/gpd.h
GPD_SCALE_*) as an autograd leaf -- run in float64 it is the reference `gpd_rollout_vjp_plant` + `gpd_plant_derive_vjp` are held
against: the cases, the metric, and the numpy float64 statement of `gpd_plant_derive` and of the transpose of its Jacobian.
Test infrastructure."""
import numpy as np

import diff_f64 as ref

SCALES = ref.SCALES

#: the gradient cases: 70 drones, task hover, cotangents on every output, make_inputs(seed=1), scales U(0.8, 1.2) rounded to fp32
CASES = {
    "rpm_k3_s1": dict(model="cf2x", act="rpm", S=1, drag=False, K=3),
    "drag_k8_s2": dict(model="cf2x", act="rpm", S=2, drag=True, K=8),
    "raw_cf2p_drag_k4": dict(model="cf2p", act="raw_rpm", S=1, drag=True, K=4),       # a third of the actions outside the clip
    "one_d_racer_k2_s8": dict(model="racer", act="one_d_rpm", S=8, drag=False, K=2),
}
#: the runs of the tests: every case with random scales, and the first one with every scale 1.0 (the NORM_GAP = +0 row)
RUNS = [(name, False) for name in CASES] + [("rpm_k3_s1", True)]


def case(name, n=70, seed=1, ones=False):
    """(cfg, K, scales [9, n] float64, every value a float32) of a case"""
    d = dict(CASES[name])
    K = d.pop("K")
    scales = np.asarray(np.random.default_rng(seed + 100).uniform(0.8, 1.2, (9, n)), dtype=np.float32).astype(np.float64)
    return ref.config(**d), K, np.ones((9, n)) if ones else scales


def scale_errors(got, want):
    """max |g - g64| / max |g64| per scale (the metric of the tests); a scale whose reference gradient is all zero is left out"""
    got = np.asarray(got, dtype=np.float64)
    return {k: float(np.abs(got[i] - want[i]).max() / np.abs(want[i]).max()) for i, k in enumerate(SCALES) if np.abs(want[i]).max() > 0}


# ---- gpd_plant_derive and the transpose of its Jacobian, numpy float64 --------------------------------------------------------------
ROWS = ("M", "inv_M", "KF", "GRAVITY", "J0", "J1", "J2", "J_INV0", "J_INV1", "J_INV2", "km_over_kf", "gnd_eff", "drag0", "drag1", "drag2",
        "hover_thrust", "hover_resid", "norm_thrust", "norm_gap")


def derive(nom, s):
    """rows [19, n] from the nominal fields (a dict of floats: M, inv_M, KF, GRAVITY, J[3], J_INV[3], km_over_kf, gnd_eff_coeff,
    drag_coeff[3], hover_thrust, hover_resid) and scales [9, n]: include/gpd.h GPD_PLANT_*, line by line"""
    m, kf, ht = s[0], s[4], nom["hover_thrust"]
    return np.stack([nom["M"] * m, nom["inv_M"] / m, nom["KF"] * kf, nom["GRAVITY"] * m,
                     nom["J"][0] * s[1], nom["J"][1] * s[2], nom["J"][2] * s[3],
                     nom["J_INV"][0] / s[1], nom["J_INV"][1] / s[2], nom["J_INV"][2] / s[3],
                     nom["km_over_kf"] * s[5] / kf, nom["gnd_eff_coeff"] * s[8],
                     nom["drag_coeff"][0] * s[6], nom["drag_coeff"][1] * s[6], nom["drag_coeff"][2] * s[7],
                     ht * m, nom["hover_resid"] * kf + (kf - m) * ht, ht * kf, (m - kf) * ht])


def derive_vjp_numeric(nom, s, g_rows):
    """J(s)^T g_rows per drone, [9, n]: the Jacobian by complex-step differentiation of `derive` (exact to rounding: every row is a
    product or a quotient), not by the formulas under test"""
    out = np.zeros_like(s)
    for k in range(9):
        z = s.astype(np.complex128)
        z[k] += 1e-30j
        out[k] = (derive(nom, z).imag / 1e-30 * g_rows).sum(axis=0)
    return out
