/*
 * Drives the HOST side of gpd_mppi_plant (include/gpd.h) under AddressSanitizer + UndefinedBehaviorSanitizer on a machine without a GPU,
 * the way tests/c/mppi_peers_host.c drives gpd_mppi_peers: libgpd's units compiled host-only with the sanitizers, the HIP runtime
 * replaced by tests/stubs/hip_stub.c (launches are counted and named, nothing runs).  Accepted arguments: one launch, its geometry (four
 * drones per workgroup of 256), and WHICH kernel (gpd_mppi_plant_kernel<ACT, OBST, EXT, PLANT>: ACT 0 RPM, 2 VEL, -1 CTBR).  Rejected
 * arguments: the code, a message that names the entry and the reason, and no launch.  Device pointers are fake non-null addresses: host
 * code must never dereference them.  One line per check; exit code = failed checks.
 */
#include <math.h>

#include "host_check.h"

static GpdParams P;
static GpdCtbr B;
static GpdState S;
static GpdStepCfg C;
static GpdMppi Q;
static const GpdCtbr* ctbr;
static const float* rows;
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
    P.pid_kf = 3.16e-10f;
    S.kin = DEV(1); S.step_counter = DEV(2); S.pid = DEV(3); S.last_rpm = DEV(10); S.ld = 128;
    C.num_envs = 70; C.drones_per_env = 1; C.act_type = GPD_ACT_VEL; C.substeps = 5; C.pyb_dt = 1.0f / 240; C.ctrl_dt = 1.0f / 48;
    C.inv_ctrl_dt = 48.0f; C.lanes_per_wave = 64; C.task = GPD_TASK_NONE;
    C.physics_flags = GPD_PHYS_GND | GPD_PHYS_DRAG;
    Q.horizon = 5; Q.samples = 192; Q.lambda = 0.5f; Q.w_pos = 1.0f; Q.w_term = 2.0f; Q.w_obs = 10.0f; Q.obst_margin = 0.3f;
    Q.collision_radius = 0.06f;
    for (int i = 0; i < 4; ++i) { Q.sigma[i] = 0.3f; Q.act_lo[i] = -1.0f; Q.act_hi[i] = 1.0f; }
    ctbr = NULL;
    rows = DEV(11);
    u_in = DEV(4); goal = DEV(5); obst = DEV(6); u_out = DEV(7); costs = DEV(8); stats = DEV(9);
    n_obst = 7; obst_ld = 70; u_stride = 70 * 4; goal_stride = 0;
}
static void use_ctbr(void) { ctbr = &B; C.act_type = GPD_ACT_DIRECT_RPM; for (int i = 0; i < 4; ++i) { Q.act_lo[i] = i ? -6.0f : 0.0f; Q.act_hi[i] = i ? 6.0f : 40.0f; } }
static int call(void) {
    return gpd_mppi_plant(&P, ctbr, &S, &C, &Q, rows, u_in, u_stride, goal, goal_stride, obst, n_obst, obst_ld, u_out, costs, stats, NULL);
}
#define REFUSED(code, reason, what) do { const int n0_ = hipstub_launches(); CHECK(refused(call(), code, "gpd_mppi_plant", reason, n0_), what); defaults(); } while (0)
#define LAUNCHES(piece, what) do { const int n0_ = hipstub_launches(); unsigned g_[7]; const int rc_ = call(); hipstub_last(g_); \
    CHECK(rc_ == 0 && hipstub_launches() == n0_ + 1 && KERNEL("gpd_mppi_plant_kernel") && KERNEL(piece) && g_[0] == 18 && g_[3] == 256, what); defaults(); } while (0)
#define NULL_ARG(expr, what) do { const int n0_ = hipstub_launches(); CHECK(refused(expr, GPD_EINVAL, "gpd_mppi_plant", "NULL", n0_), what); } while (0)

int main(void) {
    defaults();
    const float nan = __builtin_nanf("");

    /* ---- accepted: one launch of the instantiation model x list x flags x table, 70 drones in 18 workgroups of 4 waves ---- */
    LAUNCHES("ILi2ELb1ELb1ELb1E", "VEL, per-aviary lists, GND|DRAG, a table -> <VEL, OBST, EXT, PLANT>");
    obst = NULL; rows = NULL;
    LAUNCHES("ILi2ELb0ELb1ELb0E", "VEL, no list, GND|DRAG, no table -> <VEL, no OBST, EXT, no PLANT>");
    C.physics_flags = 0;
    LAUNCHES("ILi2ELb1ELb0ELb1E", "VEL, lists, no flag, a table -> <VEL, OBST, no EXT, PLANT>");
    C.physics_flags = 0; rows = NULL; S.last_rpm = NULL;
    LAUNCHES("ILi2ELb1ELb0ELb0E", "VEL, lists, no flag, no table, no state.last_rpm -> gpd_mppi's model");
    C.act_type = GPD_ACT_RPM; obst_ld = 0; n_obst = 3; C.physics_flags = GPD_PHYS_GND | GPD_PHYS_DRAG | GPD_PHYS_GROUND | GPD_PHYS_DAMP;
    LAUNCHES("ILi0ELb1ELb1ELb1E", "RPM, a shared list, the four flags, a table -> <RPM, OBST, EXT, PLANT>");
    C.act_type = GPD_ACT_RPM; n_obst = 0; S.pid = NULL; C.physics_flags = GPD_PHYS_GROUND; S.last_rpm = NULL;
    LAUNCHES("ILi0ELb0ELb1ELb1E", "RPM, no list (n_obst 0), no state.pid, the ground plane alone without state.last_rpm");
    C.act_type = GPD_ACT_RPM; C.physics_flags = 0; rows = NULL; obst = NULL;
    LAUNCHES("ILi0ELb0ELb0ELb0E", "RPM, nothing -> <RPM, no OBST, no EXT, no PLANT>");
    use_ctbr();
    LAUNCHES("ILin1ELb1ELb1ELb1E", "CTBR, per-aviary lists, GND|DRAG, a table -> <CTBR, OBST, EXT, PLANT>");
    use_ctbr(); C.act_type = GPD_ACT_RAW_RPM; obst = NULL; S.pid = NULL; rows = NULL; C.physics_flags = GPD_PHYS_DAMP;
    LAUNCHES("ILin1ELb0ELb1ELb0E", "CTBR on RAW_RPM, no list, damping, no table -> <CTBR, no OBST, EXT, no PLANT>");
    use_ctbr(); C.physics_flags = 0;
    LAUNCHES("ILin1ELb1ELb0ELb1E", "CTBR, lists, no flag, a table -> <CTBR, OBST, no EXT, PLANT>");
    use_ctbr(); C.physics_flags = 0; rows = NULL; S.last_rpm = NULL;
    LAUNCHES("ILin1ELb1ELb0ELb0E", "CTBR, lists, no flag, no table -> gpd_mppi_ctbr's model");

    /* ---- what this entry adds to the refusals ---- */
    rows = ODD(DEV(11), 4); REFUSED(GPD_EINVAL, "plant_rows", "misaligned plant_rows");
    rows = ODD(DEV(11), 8); REFUSED(GPD_EINVAL, "aligned", "plant_rows aligned to 8 bytes only");
    S.last_rpm = NULL; REFUSED(GPD_EINVAL, "last_rpm", "GPD_PHYS_DRAG without state.last_rpm");
    use_ctbr(); S.last_rpm = NULL; REFUSED(GPD_EINVAL, "last_rpm", "GPD_PHYS_DRAG without state.last_rpm, CTBR");
    for (int with = 0; with < 2; ++with) {
        if (with) use_ctbr();
        C.physics_flags = GPD_PHYS_DW; REFUSED(GPD_ENOTSUP, "downwash", "GPD_PHYS_DW alone");
        if (with) use_ctbr();
        C.physics_flags |= GPD_PHYS_DW; REFUSED(GPD_ENOTSUP, "downwash", "GPD_PHYS_DW among the other flags");
        if (with) use_ctbr();
        S.dw_force = DEV(12); REFUSED(GPD_ENOTSUP, "downwash", "state.dw_force");
    }

    /* ---- GPD_EINVAL: everything the model's own entry answers with it ---- */
    NULL_ARG(gpd_mppi_plant(NULL, NULL, &S, &C, &Q, rows, u_in, u_stride, goal, 0, obst, n_obst, obst_ld, u_out, costs, stats, NULL), "NULL params");
    NULL_ARG(gpd_mppi_plant(&P, NULL, NULL, &C, &Q, rows, u_in, u_stride, goal, 0, obst, n_obst, obst_ld, u_out, costs, stats, NULL), "NULL state");
    NULL_ARG(gpd_mppi_plant(&P, NULL, &S, NULL, &Q, rows, u_in, u_stride, goal, 0, obst, n_obst, obst_ld, u_out, costs, stats, NULL), "NULL cfg");
    NULL_ARG(gpd_mppi_plant(&P, NULL, &S, &C, NULL, rows, u_in, u_stride, goal, 0, obst, n_obst, obst_ld, u_out, costs, stats, NULL), "NULL mppi");
    u_in = NULL; REFUSED(GPD_EINVAL, "NULL", "NULL u_in");
    goal = NULL; REFUSED(GPD_EINVAL, "NULL", "NULL goal");
    u_out = NULL; REFUSED(GPD_EINVAL, "NULL", "NULL u_out");
    costs = NULL; REFUSED(GPD_EINVAL, "NULL", "NULL costs (the workspace is required)");
    stats = NULL; REFUSED(GPD_EINVAL, "NULL", "NULL stats4");
    S.kin = NULL; REFUSED(GPD_EINVAL, "NULL state.kin", "NULL state.kin");
    S.step_counter = NULL; REFUSED(GPD_EINVAL, "NULL state.kin", "NULL state.step_counter");
    S.pid = NULL; REFUSED(GPD_EINVAL, "state.pid", "VEL without state.pid");
    S.kin = ODD(DEV(1), 4); REFUSED(GPD_EINVAL, "16-byte", "misaligned state.kin");
    S.ld = 64; REFUSED(GPD_EINVAL, "state.ld", "state.ld < num_envs");
    Q.samples = 0; REFUSED(GPD_EINVAL, "samples", "samples 0");
    Q.samples = 100; REFUSED(GPD_EINVAL, "samples", "samples not a multiple of 64");
    Q.samples = 1088; REFUSED(GPD_EINVAL, "samples", "samples above 1024");
    Q.horizon = 0; REFUSED(GPD_EINVAL, "horizon", "horizon 0");
    Q.lambda = 0.0f; REFUSED(GPD_EINVAL, "lambda", "lambda 0");
    Q.lambda = nan; REFUSED(GPD_EINVAL, "lambda", "lambda NaN");
    Q.sigma[1] = -0.1f; REFUSED(GPD_EINVAL, "sigma", "a negative sigma");
    Q.sigma[3] = nan; REFUSED(GPD_EINVAL, "sigma", "a NaN sigma");
    Q.act_lo[2] = 0.5f; Q.act_hi[2] = 0.25f; REFUSED(GPD_EINVAL, "act_lo", "act_lo > act_hi");
    u_out = (float*)DEV(4); REFUSED(GPD_EINVAL, "alias", "u_out == u_in");
    u_in = ODD(DEV(4), 8); REFUSED(GPD_EINVAL, "aligned", "misaligned u_in");
    u_out = ODD(DEV(7), 4); REFUSED(GPD_EINVAL, "aligned", "misaligned u_out");
    goal = ODD(DEV(5), 12); REFUSED(GPD_EINVAL, "aligned", "misaligned goal");
    stats = ODD(DEV(9), 4); REFUSED(GPD_EINVAL, "aligned", "misaligned stats4");
    u_stride = 69 * 4; REFUSED(GPD_EINVAL, "stride", "u_step_stride below a step's rows");
    u_stride = 70 * 4 + 2; REFUSED(GPD_EINVAL, "stride", "u_step_stride not a multiple of 4");
    goal_stride = -4; REFUSED(GPD_EINVAL, "stride", "negative goal_step_stride");
    goal_stride = 8; REFUSED(GPD_EINVAL, "stride", "goal_step_stride below a step's rows");
    n_obst = -1; REFUSED(GPD_EINVAL, "n_obst", "negative n_obst");
    n_obst = GPD_OBST_MAX + 1; REFUSED(GPD_EINVAL, "n_obst", "n_obst above GPD_OBST_MAX");
    obst_ld = 69; REFUSED(GPD_EINVAL, "obst_ld", "obst_ld below num_envs");
    obst_ld = 1; REFUSED(GPD_EINVAL, "obst_ld", "obst_ld 1 (the shared list is 0 here)");
    C.num_envs = 0; REFUSED(GPD_EINVAL, "positive", "num_envs 0");
    C.substeps = 0; REFUSED(GPD_EINVAL, "positive", "substeps 0");
    C.act_type = 9; REFUSED(GPD_EINVAL, "act_type", "unknown act_type");
    C.task = 7; REFUSED(GPD_EINVAL, "task", "unknown task");
    C.physics_flags = 32; REFUSED(GPD_EINVAL, "unknown physics flag", "an unknown physics flag");

    /* ---- GPD_ENOTSUP, GPD_ERANGE: what the planning model is not, for either model ---- */
    for (int with = 0; with < 2; ++with) {
#define MODEL() do { if (with) use_ctbr(); } while (0)
        MODEL(); C.drones_per_env = 2; C.num_envs = 35; REFUSED(GPD_ENOTSUP, "drones_per_env", "aviaries of two");
        MODEL(); C.task = GPD_TASK_HOVER; REFUSED(GPD_ENOTSUP, "episode", "a task");
        MODEL(); C.auto_reset = 1; REFUSED(GPD_ENOTSUP, "episode", "auto_reset");
        for (int act = GPD_ACT_RPM; act <= GPD_ACT_DIRECT_RPM; ++act) {
            const int ctbr_act = act == GPD_ACT_RAW_RPM || act == GPD_ACT_DIRECT_RPM, own_act = act == GPD_ACT_RPM || act == GPD_ACT_VEL;
            if (with ? ctbr_act : own_act) continue;
            MODEL(); C.act_type = act; REFUSED(GPD_ENOTSUP, "act_type", "an action type of the other model or of neither");
        }
        MODEL(); C.num_envs = (1 << 26) + 1; S.ld = (1 << 26) + 64; REFUSED(GPD_ERANGE, "2^26", "more than 2^26 drones");
#undef MODEL
    }
    P.pid_kf = 0.0f; REFUSED(GPD_ENOTSUP, "DSLPID", "VEL on an airframe without DSLPID");

    printf("%d checks failed\n", failed);
    return failed;
}
