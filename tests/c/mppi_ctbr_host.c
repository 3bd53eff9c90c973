/*
 * Drives the HOST side of gpd_mppi_ctbr (include/gpd.h) under AddressSanitizer + UndefinedBehaviorSanitizer on a machine without a GPU,
 * the way tests/c/mppi_host.c drives gpd_mppi: libgpd's units compiled host-only with the sanitizers, the HIP runtime replaced by
 * tests/stubs/hip_stub.c (launches are counted and named, nothing runs).  Accepted arguments: one launch, its geometry (four drones
 * per workgroup of 256), and WHICH kernel (gpd_mppi_ctbr_kernel<OBST>).  Rejected arguments: the code, a message that names the entry
 * and the reason, and no launch.  Device pointers are fake non-null addresses: host code must never dereference them.
 * Prints one line per check; exit code = failed checks.
 */
#include "host_check.h"

static GpdParams P;
static GpdCtbr B;
static GpdState S;
static GpdStepCfg C;
static GpdMppi Q;
static const float* u_in;
static const float* goal;
static const float* obst;
static float *u_out, *costs, *stats;
static int32_t n_obst;
static int64_t obst_ld, u_stride, goal_stride;

static void defaults(void) {
    memset(&P, 0, sizeof P);
    memset(&B, 0, sizeof B);
    memset(&S, 0, sizeof S);
    memset(&C, 0, sizeof C);
    memset(&Q, 0, sizeof Q);
    S.kin = DEV(1); S.step_counter = DEV(2); S.ld = 128;          /* (no state.pid, no state.last_rpm: neither is read) */
    C.num_envs = 70; C.drones_per_env = 1; C.act_type = GPD_ACT_DIRECT_RPM; C.substeps = 5; C.pyb_dt = 1.0f / 240; C.ctrl_dt = 1.0f / 48;
    C.inv_ctrl_dt = 48.0f; C.lanes_per_wave = 64; C.task = GPD_TASK_NONE;
    Q.horizon = 5; Q.samples = 192; Q.lambda = 0.5f; Q.w_pos = 1.0f; Q.w_term = 2.0f; Q.w_obs = 10.0f; Q.obst_margin = 0.3f;
    Q.collision_radius = 0.06f;
    for (int i = 0; i < 4; ++i) { Q.sigma[i] = 2.0f; Q.act_lo[i] = i ? -6.0f : 0.0f; Q.act_hi[i] = i ? 6.0f : 40.0f; }
    u_in = DEV(4); goal = DEV(5); obst = DEV(6); u_out = DEV(7); costs = DEV(8); stats = DEV(9);
    n_obst = 7; obst_ld = 70; u_stride = 70 * 4; goal_stride = 0;
}
static int call(void) {
    return gpd_mppi_ctbr(&P, &B, &S, &C, &Q, u_in, u_stride, goal, goal_stride, obst, n_obst, obst_ld, u_out, costs, stats, NULL);
}
#define REFUSED(code, reason, what) do { const int n0_ = hipstub_launches(); CHECK(refused(call(), code, "gpd_mppi_ctbr", reason, n0_), what); defaults(); } while (0)
#define LAUNCHES(piece, what) do { const int n0_ = hipstub_launches(); unsigned g_[7]; const int rc_ = call(); hipstub_last(g_); \
    CHECK(rc_ == 0 && hipstub_launches() == n0_ + 1 && KERNEL("gpd_mppi_ctbr_kernel") && KERNEL(piece) && g_[0] == 18 && g_[3] == 256, what); defaults(); } while (0)
#define NULL_ARG(expr, what) do { const int n0_ = hipstub_launches(); CHECK(refused(expr, GPD_EINVAL, "gpd_mppi_ctbr", "NULL", n0_), what); } while (0)

int main(void) {
    defaults();

    /* ---- accepted: one launch of the variant the list selects, 70 drones in 18 workgroups of 4 waves ---- */
    LAUNCHES("ILb1E", "per-aviary lists -> <OBST>");
    obst_ld = 0; n_obst = 3;
    LAUNCHES("ILb1E", "a shared list -> <OBST>");
    obst = NULL;
    LAUNCHES("ILb0E", "no list (NULL) -> <no OBST>");
    n_obst = 0;
    LAUNCHES("ILb0E", "no list (n_obst 0) -> <no OBST>");
    C.act_type = GPD_ACT_RAW_RPM; obst = NULL; goal_stride = 70 * 4; Q.horizon = 1; u_stride = 0; Q.samples = 1024; Q.sigma[2] = 0.0f;
    LAUNCHES("ILb0E", "RAW_RPM, a goal per step, one step, 1024 samples, a zero sigma -> <no OBST>");
    Q.act_hi[0] = 100.0f; Q.act_hi[1] = 50.0f; Q.act_lo[1] = -50.0f; S.pid = DEV(3); S.last_rpm = DEV(10);
    LAUNCHES("ILb1E", "bounds beyond the controller's clips, a state with pid and last_rpm -> <OBST>");

    /* ---- GPD_EINVAL ---- */
    NULL_ARG(gpd_mppi_ctbr(NULL, &B, &S, &C, &Q, u_in, u_stride, goal, 0, obst, n_obst, obst_ld, u_out, costs, stats, NULL), "NULL params");
    NULL_ARG(gpd_mppi_ctbr(&P, NULL, &S, &C, &Q, u_in, u_stride, goal, 0, obst, n_obst, obst_ld, u_out, costs, stats, NULL), "NULL ctbr");
    NULL_ARG(gpd_mppi_ctbr(&P, &B, NULL, &C, &Q, u_in, u_stride, goal, 0, obst, n_obst, obst_ld, u_out, costs, stats, NULL), "NULL state");
    NULL_ARG(gpd_mppi_ctbr(&P, &B, &S, NULL, &Q, u_in, u_stride, goal, 0, obst, n_obst, obst_ld, u_out, costs, stats, NULL), "NULL cfg");
    NULL_ARG(gpd_mppi_ctbr(&P, &B, &S, &C, NULL, u_in, u_stride, goal, 0, obst, n_obst, obst_ld, u_out, costs, stats, NULL), "NULL mppi");
    u_in = NULL; REFUSED(GPD_EINVAL, "NULL", "NULL u_in");
    goal = NULL; REFUSED(GPD_EINVAL, "NULL", "NULL goal");
    u_out = NULL; REFUSED(GPD_EINVAL, "NULL", "NULL u_out");
    costs = NULL; REFUSED(GPD_EINVAL, "NULL", "NULL costs (the workspace is required)");
    stats = NULL; REFUSED(GPD_EINVAL, "NULL", "NULL stats4");
    S.kin = NULL; REFUSED(GPD_EINVAL, "NULL state.kin", "NULL state.kin");
    S.step_counter = NULL; REFUSED(GPD_EINVAL, "NULL state.kin", "NULL state.step_counter");
    S.kin = ODD(DEV(1), 4); REFUSED(GPD_EINVAL, "16-byte", "misaligned state.kin");
    S.ld = 64; REFUSED(GPD_EINVAL, "state.ld", "state.ld < num_envs");
    Q.samples = 0; REFUSED(GPD_EINVAL, "samples", "samples 0");
    Q.samples = 100; REFUSED(GPD_EINVAL, "samples", "samples not a multiple of 64");
    Q.samples = 1088; REFUSED(GPD_EINVAL, "samples", "samples above 1024");
    Q.horizon = 0; REFUSED(GPD_EINVAL, "horizon", "horizon 0");
    Q.lambda = 0.0f; REFUSED(GPD_EINVAL, "lambda", "lambda 0");
    Q.lambda = -1.0f; REFUSED(GPD_EINVAL, "lambda", "lambda negative");
    Q.lambda = __builtin_inff(); REFUSED(GPD_EINVAL, "lambda", "lambda infinite");
    Q.lambda = __builtin_nanf(""); REFUSED(GPD_EINVAL, "lambda", "lambda NaN");
    Q.sigma[1] = -0.1f; REFUSED(GPD_EINVAL, "sigma", "a negative sigma");
    Q.sigma[3] = __builtin_nanf(""); REFUSED(GPD_EINVAL, "sigma", "a NaN sigma");
    Q.sigma[0] = __builtin_inff(); REFUSED(GPD_EINVAL, "sigma", "an infinite sigma");
    Q.act_lo[2] = 0.5f; Q.act_hi[2] = 0.25f; REFUSED(GPD_EINVAL, "act_lo", "act_lo > act_hi");
    Q.act_lo[0] = __builtin_nanf(""); REFUSED(GPD_EINVAL, "act_lo", "a NaN bound");
    u_out = (float*)DEV(4); REFUSED(GPD_EINVAL, "alias", "u_out == u_in");
    u_in = ODD(DEV(4), 8); REFUSED(GPD_EINVAL, "aligned", "misaligned u_in");
    u_out = ODD(DEV(7), 4); REFUSED(GPD_EINVAL, "aligned", "misaligned u_out");
    goal = ODD(DEV(5), 12); REFUSED(GPD_EINVAL, "aligned", "misaligned goal");
    stats = ODD(DEV(9), 4); REFUSED(GPD_EINVAL, "aligned", "misaligned stats4");
    u_stride = 69 * 4; REFUSED(GPD_EINVAL, "stride", "u_step_stride below a step's rows");
    u_stride = 70 * 4 + 2; REFUSED(GPD_EINVAL, "stride", "u_step_stride not a multiple of 4");
    u_stride = -70 * 4; REFUSED(GPD_EINVAL, "stride", "negative u_step_stride");
    goal_stride = -4; REFUSED(GPD_EINVAL, "stride", "negative goal_step_stride");
    goal_stride = 8; REFUSED(GPD_EINVAL, "stride", "goal_step_stride below a step's rows");
    goal_stride = 70 * 4 + 1; REFUSED(GPD_EINVAL, "stride", "goal_step_stride not a multiple of 4");
    n_obst = -1; REFUSED(GPD_EINVAL, "n_obst", "negative n_obst");
    n_obst = GPD_OBST_MAX + 1; REFUSED(GPD_EINVAL, "n_obst", "n_obst above GPD_OBST_MAX");
    obst_ld = 69; REFUSED(GPD_EINVAL, "obst_ld", "obst_ld below num_envs");
    obst_ld = 1; REFUSED(GPD_EINVAL, "obst_ld", "obst_ld 1 (the shared list is 0 here)");
    obst_ld = -1; REFUSED(GPD_EINVAL, "obst_ld", "negative obst_ld");
    C.num_envs = 0; REFUSED(GPD_EINVAL, "positive", "num_envs 0");
    C.substeps = 0; REFUSED(GPD_EINVAL, "positive", "substeps 0");
    C.act_type = 9; REFUSED(GPD_EINVAL, "act_type", "unknown act_type");
    C.task = 7; REFUSED(GPD_EINVAL, "task", "unknown task");
    C.physics_flags = 32; REFUSED(GPD_EINVAL, "unknown physics flag", "an unknown physics flag");

    /* ---- GPD_ENOTSUP: what the planning model is not ---- */
    C.drones_per_env = 2; C.num_envs = 35; REFUSED(GPD_ENOTSUP, "drones_per_env", "aviaries of two");
    for (uint32_t flag = 1; flag <= 16; flag <<= 1) { C.physics_flags = flag; REFUSED(GPD_ENOTSUP, "physics_flags", "a physics flag"); }
    C.physics_flags = 3; REFUSED(GPD_ENOTSUP, "physics_flags", "two physics flags");
    C.task = GPD_TASK_HOVER; REFUSED(GPD_ENOTSUP, "episode", "a task");
    C.auto_reset = 1; REFUSED(GPD_ENOTSUP, "episode", "auto_reset");
    for (int act = GPD_ACT_RPM; act <= GPD_ACT_DIRECT_RPM; ++act) {
        if (act == GPD_ACT_RAW_RPM || act == GPD_ACT_DIRECT_RPM) continue;
        C.act_type = act; REFUSED(GPD_ENOTSUP, "act_type", "another action type");
    }
    C.num_envs = (1 << 26) + 1; S.ld = (1 << 26) + 64; REFUSED(GPD_ERANGE, "2^26", "more than 2^26 drones");

    printf("%d checks failed\n", failed);
    return failed;
}
