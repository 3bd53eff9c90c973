/*
 * Drives the HOST side of gpd_mppi (include/gpd.h) under AddressSanitizer + UndefinedBehaviorSanitizer on a machine without a GPU, the
 * way tests/c/diff_host.c drives the differentiable rollout: libgpd's units compiled host-only with the sanitizers, the HIP runtime
 * replaced by tests/stubs/hip_stub.c (launches are counted and named, nothing runs).  Accepted arguments: one launch, its geometry (four
 * drones per workgroup of 256), and WHICH kernel (gpd_mppi_kernel<ACT, OBST>).  Rejected arguments: the code, a message that names the
 * entry and the reason, and no launch.  Device pointers are fake non-null addresses: host code must never dereference them.
 * It also evaluates csrc/mppi_math.inc -- the text the device kernel compiles:
 *   mppi_host philox  IN OUT     IN: int32 count, then count x (4 counter words, 2 key words); OUT: count x 4 words
 *   mppi_host normals N M H ITERATION SEED0 SEED1 OUT     OUT: [N][M][H][4] floats, the normals of gpd_mppi_normals
 * Prints one line per check; exit code = failed checks.
 */
#define _GNU_SOURCE      /* sincosf */
#include <stdlib.h>

#include "host_check.h"
#include "mppi_math.inc"

static GpdParams P;
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
    memset(&S, 0, sizeof S);
    memset(&C, 0, sizeof C);
    memset(&Q, 0, sizeof Q);
    P.pid_kf = 3.16e-10f;
    S.kin = DEV(1); S.step_counter = DEV(2); S.pid = DEV(3); S.ld = 128;
    C.num_envs = 70; C.drones_per_env = 1; C.act_type = GPD_ACT_VEL; C.substeps = 5; C.pyb_dt = 1.0f / 240; C.ctrl_dt = 1.0f / 48;
    C.inv_ctrl_dt = 48.0f; C.lanes_per_wave = 64; C.task = GPD_TASK_NONE;
    Q.horizon = 5; Q.samples = 192; Q.lambda = 0.5f; Q.w_pos = 1.0f; Q.w_term = 2.0f; Q.w_obs = 10.0f; Q.obst_margin = 0.3f;
    Q.collision_radius = 0.06f;
    for (int i = 0; i < 4; ++i) { Q.sigma[i] = 0.3f; Q.act_lo[i] = -1.0f; Q.act_hi[i] = 1.0f; }
    u_in = DEV(4); goal = DEV(5); obst = DEV(6); u_out = DEV(7); costs = DEV(8); stats = DEV(9);
    n_obst = 7; obst_ld = 70; u_stride = 70 * 4; goal_stride = 0;
}
static int call(void) {
    return gpd_mppi(&P, &S, &C, &Q, u_in, u_stride, goal, goal_stride, obst, n_obst, obst_ld, u_out, costs, stats, NULL);
}
#define REFUSED(code, reason, what) do { const int n0_ = hipstub_launches(); CHECK(refused(call(), code, "gpd_mppi", reason, n0_), what); defaults(); } while (0)
#define LAUNCHES(piece, what) do { const int n0_ = hipstub_launches(); unsigned g_[7]; const int rc_ = call(); hipstub_last(g_); \
    CHECK(rc_ == 0 && hipstub_launches() == n0_ + 1 && KERNEL("gpd_mppi_kernel") && KERNEL(piece) && g_[0] == 18 && g_[3] == 256, what); defaults(); } while (0)

static int write_philox(const char* in, const char* out) {
    FILE* f = fopen(in, "rb");
    int32_t count = 0;
    if (!f || fread(&count, 4, 1, f) != 1 || count < 0) return 1;
    uint32_t* w = malloc((size_t)count * 6 * 4 + 4);
    uint32_t* o = malloc((size_t)count * 4 * 4 + 4);
    if (!w || !o || fread(w, 24, (size_t)count, f) != (size_t)count) return 1;
    fclose(f);
    for (int32_t i = 0; i < count; ++i)
        gpd_philox4x32(w[6 * i], w[6 * i + 1], w[6 * i + 2], w[6 * i + 3], w[6 * i + 4], w[6 * i + 5], &o[4 * i], &o[4 * i + 1], &o[4 * i + 2], &o[4 * i + 3]);
    f = fopen(out, "wb");
    if (!f || fwrite(o, 16, (size_t)count, f) != (size_t)count) return 1;
    free(w);
    free(o);
    return fclose(f) != 0;
}

static int write_normals(char** a) {
    const uint32_t N = (uint32_t)strtoul(a[0], NULL, 0), M = (uint32_t)strtoul(a[1], NULL, 0), H = (uint32_t)strtoul(a[2], NULL, 0);
    const uint32_t it = (uint32_t)strtoul(a[3], NULL, 0), s0 = (uint32_t)strtoul(a[4], NULL, 0), s1 = (uint32_t)strtoul(a[5], NULL, 0);
    FILE* f = fopen(a[6], "wb");
    if (!f) return 1;
    for (uint32_t n = 0; n < N; ++n)
        for (uint32_t m = 0; m < M; ++m)
            for (uint32_t h = 0; h < H; ++h) {
                float z[4];
                gpd_mppi_normals(n, m, h, it, s0, s1, &z[0], &z[1], &z[2], &z[3]);
                if (fwrite(z, 4, 4, f) != 4) return 1;
            }
    return fclose(f) != 0;
}

int main(int argc, char** argv) {
    if (argc == 4 && strcmp(argv[1], "philox") == 0) return write_philox(argv[2], argv[3]);
    if (argc == 9 && strcmp(argv[1], "normals") == 0) return write_normals(argv + 2);
    defaults();

    /* ---- accepted: one launch of the variant the action type and the list select, 70 drones in 18 workgroups of 4 waves ---- */
    LAUNCHES("ILi2ELb1E", "VEL with per-aviary lists -> <VEL, OBST>");
    obst_ld = 0; n_obst = 3;
    LAUNCHES("ILi2ELb1E", "VEL with a shared list -> <VEL, OBST>");
    obst = NULL;
    LAUNCHES("ILi2ELb0E", "VEL without a list (NULL) -> <VEL, no OBST>");
    n_obst = 0;
    LAUNCHES("ILi2ELb0E", "VEL without a list (n_obst 0) -> <VEL, no OBST>");
    C.act_type = GPD_ACT_RPM; S.pid = NULL;
    LAUNCHES("ILi0ELb1E", "RPM (no state.pid needed) -> <RPM, OBST>");
    C.act_type = GPD_ACT_RPM; obst = NULL; goal_stride = 70 * 4; Q.horizon = 1; u_stride = 0; Q.samples = 1024; Q.sigma[2] = 0.0f;
    LAUNCHES("ILi0ELb0E", "RPM, a goal per step, one step, 1024 samples, a zero sigma -> <RPM, no OBST>");

    /* ---- GPD_EINVAL ---- */
    u_in = NULL; REFUSED(GPD_EINVAL, "NULL", "NULL u_in");
    goal = NULL; REFUSED(GPD_EINVAL, "NULL", "NULL goal");
    u_out = NULL; REFUSED(GPD_EINVAL, "NULL", "NULL u_out");
    costs = NULL; REFUSED(GPD_EINVAL, "NULL", "NULL costs (the workspace is required)");
    stats = NULL; REFUSED(GPD_EINVAL, "NULL", "NULL stats4");
    S.kin = NULL; REFUSED(GPD_EINVAL, "NULL state.kin", "NULL state.kin");
    { const int n0 = hipstub_launches(); CHECK(refused(gpd_mppi(&P, &S, &C, NULL, u_in, u_stride, goal, 0, obst, n_obst, obst_ld, u_out, costs, stats, NULL), GPD_EINVAL, "gpd_mppi", "NULL", n0), "NULL mppi"); }
    { const int n0 = hipstub_launches(); CHECK(refused(gpd_mppi(NULL, &S, &C, &Q, u_in, u_stride, goal, 0, obst, n_obst, obst_ld, u_out, costs, stats, NULL), GPD_EINVAL, "gpd_mppi", "NULL", n0), "NULL params"); }
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
    obst_ld = -1; REFUSED(GPD_EINVAL, "obst_ld", "negative obst_ld");
    S.pid = NULL; REFUSED(GPD_EINVAL, "state.pid", "VEL without state.pid");
    C.substeps = 0; REFUSED(GPD_EINVAL, "positive", "substeps 0");
    C.act_type = 9; REFUSED(GPD_EINVAL, "act_type", "unknown act_type");

    /* ---- GPD_ENOTSUP: what the planning model is not ---- */
    C.drones_per_env = 2; C.num_envs = 35; REFUSED(GPD_ENOTSUP, "drones_per_env", "aviaries of two");
    for (uint32_t flag = 1; flag <= 16; flag <<= 1) { C.physics_flags = flag; REFUSED(GPD_ENOTSUP, "physics_flags", "a physics flag"); }
    C.task = GPD_TASK_HOVER; REFUSED(GPD_ENOTSUP, "episode", "a task");
    C.auto_reset = 1; REFUSED(GPD_ENOTSUP, "episode", "auto_reset");
    for (int act = GPD_ACT_RPM; act <= GPD_ACT_DIRECT_RPM; ++act) {
        if (act == GPD_ACT_RPM || act == GPD_ACT_VEL) continue;
        C.act_type = act; REFUSED(GPD_ENOTSUP, "act_type", "another action type");
    }
    P.pid_kf = 0.0f; REFUSED(GPD_ENOTSUP, "DSLPID", "VEL on an airframe without DSLPID");
    C.num_envs = (1 << 26) + 1; S.ld = (1 << 26) + 64; REFUSED(GPD_ERANGE, "2^26", "more than 2^26 drones");

    /* ---- mppi_math.inc: the documented corner values ---- */
    {
        uint32_t o[4];
        gpd_philox4x32(0, 0, 0, 0, 0, 0, &o[0], &o[1], &o[2], &o[3]);
        CHECK(o[0] == 0x6627e8d5u && o[1] == 0xe169c58du && o[2] == 0xbc57ac4cu && o[3] == 0x9b00dbd8u, "Philox4x32-10 of zeros");
        CHECK(gpd_mppi_uniform(0u) == 0.5f * 5.9604644775390625e-8f && gpd_mppi_uniform(0xffffffffu) == 1.0f && gpd_mppi_uniform(0x7fffffffu) < 1.0f,
              "the uniforms' ends: 2^-25 and (rounded) 1");
        float z0, z1;
        gpd_mppi_box_muller(1.0f, 0.25f, &z0, &z1);
        CHECK(z0 == 0.0f && z1 == 0.0f, "u1 = 1 gives r = 0, not a NaN");
        CHECK(gpd_mppi_perturb(0.3f, 0.0f, 123.0f, -1.0f, 1.0f) == 0.3f && gpd_mppi_perturb(1.5f, 0.0f, -7.0f, -1.0f, 1.0f) == 1.0f, "sigma 0: clamp(u)");
        CHECK(gpd_mppi_weight(__builtin_nanf(""), 1.0f, 2.0f) == 0.0f && gpd_mppi_weight(__builtin_inff(), 1.0f, 2.0f) == 0.0f &&
              gpd_mppi_weight(1.0f, 1.0f, 2.0f) == 1.0f, "weights: 0 for a cost that is not finite, 1 at the minimum");
        CHECK(gpd_mppi_step_cost(1.0f, 0.0f, 0.0f, 0.0f, 5.0f, 0.3f, 0.06f, 2.0f, 9.0f, 9.0f, 9.0f, __builtin_inff()) == 2.0f, "no obstacle near: no hinge");
        CHECK(gpd_mppi_step_cost(0.0f, 0.0f, 0.0f, 0.0f, 4.0f, 0.5f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.25f) == 0.25f, "the hinge: w_obs (margin - d)^2");
    }
    printf("%d checks failed\n", failed);
    return failed;
}
