/*
 * Drives the HOST side of gpd_mppi_peers (include/gpd.h) under AddressSanitizer + UndefinedBehaviorSanitizer on a machine without a GPU,
 * the way tests/c/mppi_ctbr_host.c drives gpd_mppi_ctbr: libgpd's units compiled host-only with the sanitizers, the HIP runtime replaced
 * by tests/stubs/hip_stub.c (launches are counted and named, nothing runs).  Accepted arguments: one launch, its geometry (four drones
 * per workgroup of 256), and WHICH kernel (gpd_mppi_peers_kernel<ACT, OBST>: ACT 0 RPM, 2 VEL, -1 CTBR).  Rejected arguments: the code,
 * a message that names the entry and the reason, and no launch.  Device pointers are fake non-null addresses: host code must never
 * dereference them.
 * It also evaluates csrc/mppi_peers_math.inc -- the text the device kernel compiles -- at corner values, one line each:
 *   pen PEER_DIST DX DY DZ -> PEN DISTANCE NEAREST        (NEAREST: gpd_mppi_peer_nearest(DISTANCE, 1.0f))
 * and prints sizeof(GpdMppiPeers).  One line per check; exit code = failed checks.
 */
#include <math.h>

#include "host_check.h"
#include "mppi_peers_math.inc"

static GpdParams P;
static GpdCtbr B;
static GpdState S;
static GpdStepCfg C;
static GpdMppi Q;
static GpdMppiPeers R;
static const GpdCtbr* ctbr;
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
    memset(&R, 0, sizeof R);
    P.pid_kf = 3.16e-10f;
    S.kin = DEV(1); S.step_counter = DEV(2); S.pid = DEV(3); S.ld = 128;
    C.num_envs = 70; C.drones_per_env = 1; C.act_type = GPD_ACT_VEL; C.substeps = 5; C.pyb_dt = 1.0f / 240; C.ctrl_dt = 1.0f / 48;
    C.inv_ctrl_dt = 48.0f; C.lanes_per_wave = 64; C.task = GPD_TASK_NONE;
    Q.horizon = 5; Q.samples = 192; Q.lambda = 0.5f; Q.w_pos = 1.0f; Q.w_term = 2.0f; Q.w_obs = 10.0f; Q.obst_margin = 0.3f;
    Q.collision_radius = 0.06f;
    for (int i = 0; i < 4; ++i) { Q.sigma[i] = 0.3f; Q.act_lo[i] = -1.0f; Q.act_hi[i] = 1.0f; }
    R.idx = DEV(11); R.pos = DEV(12); R.path_out = DEV(13); R.k = 8; R.idx_ld = 10; R.n_rows = 73; R.pos_step_stride = 76 * 4;
    R.w_peer = 100.0f; R.peer_dist = 0.4f;
    ctbr = NULL;
    u_in = DEV(4); goal = DEV(5); obst = DEV(6); u_out = DEV(7); costs = DEV(8); stats = DEV(9);
    n_obst = 7; obst_ld = 70; u_stride = 70 * 4; goal_stride = 0;
}
static void use_ctbr(void) { ctbr = &B; C.act_type = GPD_ACT_DIRECT_RPM; for (int i = 0; i < 4; ++i) { Q.act_lo[i] = i ? -6.0f : 0.0f; Q.act_hi[i] = i ? 6.0f : 40.0f; } }
static int call(void) {
    return gpd_mppi_peers(&P, ctbr, &S, &C, &Q, &R, u_in, u_stride, goal, goal_stride, obst, n_obst, obst_ld, u_out, costs, stats, NULL);
}
#define REFUSED(code, reason, what) do { const int n0_ = hipstub_launches(); CHECK(refused(call(), code, "gpd_mppi_peers", reason, n0_), what); defaults(); } while (0)
#define LAUNCHES(piece, what) do { const int n0_ = hipstub_launches(); unsigned g_[7]; const int rc_ = call(); hipstub_last(g_); \
    CHECK(rc_ == 0 && hipstub_launches() == n0_ + 1 && KERNEL("gpd_mppi_peers_kernel") && KERNEL(piece) && g_[0] == 18 && g_[3] == 256, what); defaults(); } while (0)
#define NULL_ARG(expr, what) do { const int n0_ = hipstub_launches(); CHECK(refused(expr, GPD_EINVAL, "gpd_mppi_peers", "NULL", n0_), what); } while (0)

static void pen_line(float peer_dist, float dx, float dy, float dz) {
    const float d = gpd_mppi_peer_distance(dx, dy, dz);
    printf("pen %a %a %a %a -> %a %a %a\n", (double)peer_dist, (double)dx, (double)dy, (double)dz, (double)gpd_mppi_peer_pen(peer_dist, dx, dy, dz), (double)d,
           (double)gpd_mppi_peer_nearest(d, 1.0f));
}

int main(void) {
    defaults();
    printf("sizeof GpdMppiPeers %zu\n", sizeof(GpdMppiPeers));

    /* ---- the hinge at its corners: d = 0, d = peer_dist (3-4-5 and 0.3-0.4-0.5 offsets), either side of it, NaN, infinities ---- */
    const float nan = __builtin_nanf(""), inf = __builtin_inff();
    pen_line(0.5f, 0.0f, 0.0f, 0.0f);
    pen_line(5.0f, 3.0f, -4.0f, 0.0f);
    pen_line(0.5f, 0.0f, 0.3f, 0.4f);
    pen_line(0.5f, 0.0f, 0.3f, 0.39999f);
    pen_line(0.5f, 0.0f, 0.3f, 0.40001f);
    pen_line(0.5f, 0.1f, -0.2f, 0.05f);
    pen_line(0.5f, 1.0f, 2.0f, 3.0f);
    pen_line(0.0f, 0.0f, 0.0f, 0.0f);
    pen_line(0.5f, nan, 0.0f, 0.0f);
    pen_line(0.5f, 0.0f, nan, 0.1f);
    pen_line(0.5f, 0.0f, 0.0f, nan);
    pen_line(0.5f, inf, 0.0f, 0.0f);
    pen_line(0.5f, -inf, inf, 0.0f);
    pen_line(0.5f, 0.0f, 0.0f, -inf);
    pen_line(0.5f, 1e30f, 1e30f, 0.0f);          /* the squares overflow: the distance is +inf, the hinge 0 */
    CHECK(gpd_mppi_peer_pen(0.5f, nan, 0.0f, 0.0f) == 0.0f && gpd_mppi_peer_pen(0.5f, inf, 0.0f, 0.0f) == 0.0f, "a row that is not finite gives 0");
    CHECK(gpd_mppi_peer_pen(0.5f, 0.0f, 0.0f, 0.0f) == 0.25f, "a peer at the drone's own point gives peer_dist^2");
    CHECK(gpd_mppi_peer_nearest(nan, GPD_OBST_INF) == GPD_OBST_INF && gpd_mppi_peer_nearest(inf, GPD_OBST_INF) == GPD_OBST_INF &&
          gpd_mppi_peer_nearest(0.25f, GPD_OBST_INF) == 0.25f && gpd_mppi_peer_nearest(nan, 0.25f) == 0.25f, "the nearest distance does not count a NaN");

    /* ---- accepted: one launch of the instantiation model x list, 70 drones in 18 workgroups of 4 waves ---- */
    LAUNCHES("ILi2ELb1E", "VEL, per-aviary lists -> <VEL, OBST>");
    obst = NULL;
    LAUNCHES("ILi2ELb0E", "VEL, no list -> <VEL, no OBST>");
    C.act_type = GPD_ACT_RPM; obst_ld = 0; n_obst = 3;
    LAUNCHES("ILi0ELb1E", "RPM, a shared list -> <RPM, OBST>");
    C.act_type = GPD_ACT_RPM; n_obst = 0; S.pid = NULL;
    LAUNCHES("ILi0ELb0E", "RPM, no list (n_obst 0), no state.pid -> <RPM, no OBST>");
    use_ctbr();
    LAUNCHES("ILin1ELb1E", "CTBR, per-aviary lists -> <CTBR, OBST>");
    use_ctbr(); C.act_type = GPD_ACT_RAW_RPM; obst = NULL; S.pid = NULL;
    LAUNCHES("ILin1ELb0E", "CTBR on RAW_RPM, no list -> <CTBR, no OBST>");
    R.path_out = NULL; R.pos_step_stride = 0; R.k = 32; R.idx_ld = 32; R.n_rows = 70; R.w_peer = 0.0f; R.peer_dist = 0.0f;
    LAUNCHES("ILi2ELb1E", "no path_out, one row set, k = idx_ld = 32, n_rows = N, zero weight and distance");
    R.k = 1; R.idx_ld = 1; R.pos_step_stride = 73 * 4;
    LAUNCHES("ILi2ELb1E", "k = idx_ld = 1, the smallest step stride");

    /* ---- GPD_EINVAL: the peers ---- */
    NULL_ARG(gpd_mppi_peers(&P, NULL, &S, &C, &Q, NULL, u_in, u_stride, goal, 0, obst, n_obst, obst_ld, u_out, costs, stats, NULL), "NULL peers");
    R.idx = NULL; REFUSED(GPD_EINVAL, "NULL", "NULL peers.idx");
    R.pos = NULL; REFUSED(GPD_EINVAL, "NULL", "NULL peers.pos");
    R.k = 0; REFUSED(GPD_EINVAL, "peers.k", "k 0");
    R.k = -1; REFUSED(GPD_EINVAL, "peers.k", "k negative");
    R.k = 33; R.idx_ld = 40; REFUSED(GPD_EINVAL, "peers.k", "k above 32");
    R.idx_ld = 7; REFUSED(GPD_EINVAL, "idx_ld", "idx_ld below k");
    R.n_rows = 69; REFUSED(GPD_EINVAL, "n_rows", "n_rows below N");
    R.pos_step_stride = 72 * 4; REFUSED(GPD_EINVAL, "pos_step_stride", "pos_step_stride below a step's rows");
    R.pos_step_stride = 76 * 4 + 2; REFUSED(GPD_EINVAL, "pos_step_stride", "pos_step_stride not a multiple of 4");
    R.pos_step_stride = -76 * 4; REFUSED(GPD_EINVAL, "pos_step_stride", "negative pos_step_stride");
    R.pos = ODD(DEV(12), 4); REFUSED(GPD_EINVAL, "aligned", "misaligned peers.pos");
    R.path_out = ODD(DEV(13), 8); REFUSED(GPD_EINVAL, "aligned", "misaligned peers.path_out");
    R.path_out = (float*)DEV(4); REFUSED(GPD_EINVAL, "alias", "path_out == u_in");
    R.path_out = (float*)DEV(7); REFUSED(GPD_EINVAL, "alias", "path_out == u_out");
    R.w_peer = -1.0f; REFUSED(GPD_EINVAL, "w_peer", "a negative w_peer");
    R.w_peer = nan; REFUSED(GPD_EINVAL, "w_peer", "a NaN w_peer");
    R.w_peer = inf; REFUSED(GPD_EINVAL, "w_peer", "an infinite w_peer");
    R.peer_dist = -0.1f; REFUSED(GPD_EINVAL, "peer_dist", "a negative peer_dist");
    R.peer_dist = nan; REFUSED(GPD_EINVAL, "peer_dist", "a NaN peer_dist");
    R.peer_dist = inf; REFUSED(GPD_EINVAL, "peer_dist", "an infinite peer_dist");

    /* ---- GPD_EINVAL: everything the model's own entry answers with it ---- */
    NULL_ARG(gpd_mppi_peers(NULL, NULL, &S, &C, &Q, &R, u_in, u_stride, goal, 0, obst, n_obst, obst_ld, u_out, costs, stats, NULL), "NULL params");
    NULL_ARG(gpd_mppi_peers(&P, NULL, NULL, &C, &Q, &R, u_in, u_stride, goal, 0, obst, n_obst, obst_ld, u_out, costs, stats, NULL), "NULL state");
    NULL_ARG(gpd_mppi_peers(&P, NULL, &S, NULL, &Q, &R, u_in, u_stride, goal, 0, obst, n_obst, obst_ld, u_out, costs, stats, NULL), "NULL cfg");
    NULL_ARG(gpd_mppi_peers(&P, NULL, &S, &C, NULL, &R, u_in, u_stride, goal, 0, obst, n_obst, obst_ld, u_out, costs, stats, NULL), "NULL mppi");
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
        for (uint32_t flag = 1; flag <= 16; flag <<= 1) { MODEL(); C.physics_flags = flag; REFUSED(GPD_ENOTSUP, "physics_flags", "a physics flag"); }
        MODEL(); C.task = GPD_TASK_HOVER; REFUSED(GPD_ENOTSUP, "episode", "a task");
        MODEL(); C.auto_reset = 1; REFUSED(GPD_ENOTSUP, "episode", "auto_reset");
        for (int act = GPD_ACT_RPM; act <= GPD_ACT_DIRECT_RPM; ++act) {
            const int ctbr_act = act == GPD_ACT_RAW_RPM || act == GPD_ACT_DIRECT_RPM, own_act = act == GPD_ACT_RPM || act == GPD_ACT_VEL;
            if (with ? ctbr_act : own_act) continue;
            MODEL(); C.act_type = act; REFUSED(GPD_ENOTSUP, "act_type", "an action type of the other model or of neither");
        }
        MODEL(); C.num_envs = (1 << 26) + 1; S.ld = (1 << 26) + 64; R.n_rows = (1 << 26) + 1; REFUSED(GPD_ERANGE, "2^26", "more than 2^26 drones");
#undef MODEL
    }
    P.pid_kf = 0.0f; REFUSED(GPD_ENOTSUP, "DSLPID", "VEL on an airframe without DSLPID");

    printf("%d checks failed\n", failed);
    return failed;
}
