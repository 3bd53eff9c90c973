/*
 * Drives the HOST side of the three entries of the differentiable rollout on thrust and body-rate commands (include/gpd.h:
 * gpd_rollout_tape_ctbr_floats, gpd_rollout_tape_ctbr, gpd_rollout_vjp_ctbr) under AddressSanitizer + UndefinedBehaviorSanitizer on a
 * machine without a GPU, the way tests/c/ctbr_host.c drives gpd_rollout_ctbr: libgpd's units compiled host-only with the sanitizers, the
 * HIP runtime replaced by tests/stubs/hip_stub.c (launches are counted and named, nothing runs).  Accepted arguments: the tape's size, one
 * launch each, its geometry, and WHICH kernel (gpd_rollout_tape_ctbr_kernel<MODE, PLANT>, gpd_rollout_vjp_ctbr_kernel<MODE, PLANT, GG>).
 * Rejected arguments: the code, a message that names the entry and the reason, and no launch.  Device pointers are fake addresses.
 * It also evaluates csrc/ctbr_vjp.inc -- the text the device sweep compiles -- in fp32:
 *   diff_ctbr_host rate IN OUT    IN: int32 count, a GpdCtbr, M Jx Jy Jz KF_plant, then count x 12 floats (command 4 | body rates 3 |
 *                                 cotangents of the four thrust deviations | plain: 1 = far from every select);
 *                                 OUT: count x 10 floats (cotangents of the command 4 | of the body rates 3 | of k_rate 3)
 *   diff_ctbr_host outer IN OUT   IN: int32 count, a GpdCtbr, then count x 21 floats (pos 3 | quat xyzw 4 | vel 3 | target pos 3 |
 *                                 target vel 3 | the command's cotangent 4 | plain);
 *                                 OUT: count x 25 floats (pos 3 | quat 4 | vel 3 | target pos 3 | target vel 3 | k_p k_d k_rates 9)
 * Both modes also hold the adjoint text against the FORWARD text (ctbr_math.inc) on the plain rows: for a direction u the program
 * draws, <v, J u> with J u by central differences of the forward text, accumulated in double, equals <J^T v, u> by the adjoint text.
 * The forward text is fp32 (values of relative noise 2^-24), so the step is 2^-7 of an input's scale: truncation of the order 2^-14 of
 * the curvature plus noise of the order 2^-24 / 2^-7 = 2^-17 of a value, against a bound of 5e-3 of sum |v_i (J u)_i|.  A mismatch, or
 * cotangents that change with the optional gain output, is a non-zero exit code.
 * Prints one line per check; exit code = failed checks.
 */
#include <stdlib.h>

#include "host_check.h"
#include "ctbr_math.inc"
#include "ctbr_vjp.inc"

static GpdParams P;
static GpdCtbr B;
static GpdState S;
static GpdStepCfg C;
static const float *rows, *plant, *tape_in, *g_obs;
static float *obs, *cmd_out, *tape, *g_kin, *g_rows, *g_gains;
static int32_t mode, K;
static int64_t rstride, ostride, ld;

static void defaults(void) {
    memset(&P, 0, sizeof P);
    memset(&B, 0, sizeof B);
    memset(&S, 0, sizeof S);
    memset(&C, 0, sizeof C);
    S.kin = DEV(1); S.step_counter = DEV(2); S.last_rpm = DEV(3); S.ld = 128; ld = 128;
    C.num_envs = 70; C.drones_per_env = 1; C.act_type = GPD_ACT_DIRECT_RPM; C.substeps = 5; C.pyb_dt = 1.0f / 240; C.ctrl_dt = 1.0f / 48;
    C.inv_ctrl_dt = 48.0f; C.lanes_per_wave = 64; C.task = GPD_TASK_NONE;
    rows = DEV(4); plant = NULL; obs = DEV(5); cmd_out = NULL; tape = DEV(10); tape_in = DEV(10); g_obs = DEV(11);
    g_kin = DEV(12); g_rows = DEV(13); g_gains = NULL;
    mode = GPD_CTBR_CMD; K = 8; rstride = 70 * 4; ostride = 70 * 12;
}
static int tape_call(void) { return gpd_rollout_tape_ctbr(&P, &B, &S, &C, mode, rows, rstride, plant, obs, ostride, cmd_out, K, tape, NULL); }
static int vjp_call(void) {
    return gpd_rollout_vjp_ctbr(&P, &B, &C, ld, mode, K, rows, rstride, plant, tape_in, g_obs, ostride, g_kin, g_rows, g_gains, NULL);
}
static int floats_call(void) { int64_t floats; return gpd_rollout_tape_ctbr_floats(&C, K, ld, &floats); }
static const struct { const char* name; int (*call)(void); } ENTRIES[3] = {
    {"gpd_rollout_tape_ctbr", tape_call}, {"gpd_rollout_vjp_ctbr", vjp_call}, {"gpd_rollout_tape_ctbr_floats", floats_call}};
/* the first `entries` of them refuse the configuration as it stands: the code, the entry and the reason, nothing launched */
static void all_refuse(int entries, int code, const char* reason, const char* what) {
    char line[160];
    for (int e = 0; e < entries; ++e) {
        const int n0 = hipstub_launches();
        snprintf(line, sizeof line, "%s: %s", ENTRIES[e].name, what);
        CHECK(refused(ENTRIES[e].call(), code, ENTRIES[e].name, reason, n0), line);
    }
    defaults();
}
#define ONE_REFUSES(e, code, reason, what) do { const int n0_ = hipstub_launches(); CHECK(refused(ENTRIES[e].call(), code, ENTRIES[e].name, reason, n0_), what); defaults(); } while (0)
#define LAUNCHES(e, kernel, piece, what) do { const int n0_ = hipstub_launches(); unsigned g_[7]; const int rc_ = ENTRIES[e].call(); hipstub_last(g_); \
    CHECK(rc_ == 0 && hipstub_launches() == n0_ + 1 && KERNEL(kernel) && KERNEL(piece) && g_[0] == 1 && g_[3] == 256, what); defaults(); } while (0)

static double draw(uint64_t* x) { *x = *x * 6364136223846793005ull + 1442695040888963407ull; return (double)(*x >> 11) / 9007199254740992.0; }

static float* read_block(const char* path, int32_t* count, GpdCtbr* b, float* extra, int n_extra, int width) {
    FILE* f = fopen(path, "rb");
    if (!f || fread(count, 4, 1, f) != 1 || *count < 0 || fread(b, sizeof *b, 1, f) != 1) return NULL;
    if (n_extra && fread(extra, 4, (size_t)n_extra, f) != (size_t)n_extra) return NULL;
    float* v = malloc((size_t)*count * (size_t)width * 4 + 4);
    if (!v || fread(v, (size_t)width * 4, (size_t)*count, f) != (size_t)*count) return NULL;
    fclose(f);
    return v;
}
static int write_block(const char* path, const float* o, int32_t count, int width) {
    FILE* f = fopen(path, "wb");
    if (!f || fwrite(o, (size_t)width * 4, (size_t)count, f) != (size_t)count) return 1;
    return fclose(f) != 0;
}

#define STEP (1.0 / 128)
#define TRANSPOSE_TOL 5e-3

/* rate loop: x = (command 4 | body rates 3) -> g_i = KF_plant rpm_i^2 (the thrust deviation but for a constant) */
static void rate_forward(const GpdCtbr* b, const float* mj, const float* x, double g[4]) {
    float rpm[4];
    gpd_ctbr_rate_loop(b, mj[0], mj[1], mj[2], mj[3], x, x[4], x[5], x[6], rpm);
    for (int i = 0; i < 4; ++i) g[i] = (double)mj[4] * (double)rpm[i] * (double)rpm[i];
}

static int write_rate(const char* in, const char* out) {
    int32_t count = 0, checked = 0;
    GpdCtbr b;
    float mj[5];
    float* v = read_block(in, &count, &b, mj, 5, 12);
    float* o = calloc((size_t)count * 10 + 1, 4);
    if (!v || !o) return 1;
    uint64_t seed = 77;
    double worst = 0.0;
    int bad = 0;
    const double scale[7] = {4.0, 1.0, 1.0, 1.0, 1.0, 1.0, 1.0};
    for (int32_t i = 0; i < count; ++i) {
        const float* r = v + 12 * i;
        float* acmd = o + 10 * i;
        gpd_ctbr_rate_loop_vjp(&b, mj[0], mj[1], mj[2], mj[3], mj[4], r, r[4], r[5], r[6], r + 7, acmd, acmd + 4, acmd + 7);
        float again[7] = {0};
        gpd_ctbr_rate_loop_vjp(&b, mj[0], mj[1], mj[2], mj[3], mj[4], r, r[4], r[5], r[6], r + 7, again, again + 4, NULL);
        if (memcmp(again, acmd, sizeof again) != 0) bad |= 2;
        if (r[11] != 1.0f) continue;
        float lo[7], hi[7];
        double u[7], glo[4], ghi[4], lhs = 0.0, rhs = 0.0, mag = 0.0;
        for (int k = 0; k < 7; ++k) { u[k] = scale[k] * (2.0 * draw(&seed) - 1.0); lo[k] = (float)(r[k] - STEP * u[k]); hi[k] = (float)(r[k] + STEP * u[k]); }
        rate_forward(&b, mj, lo, glo);
        rate_forward(&b, mj, hi, ghi);
        for (int k = 0; k < 4; ++k) { const double ju = (ghi[k] - glo[k]) / (2.0 * STEP); lhs += r[7 + k] * ju; mag += fabs(r[7 + k] * ju); }
        for (int k = 0; k < 7; ++k) rhs += (double)acmd[k] * u[k];
        const double miss = fabs(lhs - rhs) / (mag + 1e-300);
        if (miss > worst) worst = miss;
        ++checked;
    }
    printf("rate loop: <v, J u> against <J^T v, u> on %d plain rows of %d, worst mismatch %.3g of sum |v_i (J u)_i| (bound %.3g)\n", checked, count, worst, TRANSPOSE_TOL);
    if (!(worst <= TRANSPOSE_TOL) || checked < count / 8) bad |= 4;
    const int rc = write_block(out, o, count, 10);
    free(v);
    free(o);
    return rc | bad;
}

static int write_outer(const char* in, const char* out) {
    int32_t count = 0, checked = 0;
    GpdCtbr b;
    float* v = read_block(in, &count, &b, NULL, 0, 21);
    float* o = calloc((size_t)count * 25 + 1, 4);
    if (!v || !o) return 1;
    uint64_t seed = 78;
    double worst = 0.0;
    int bad = 0;
    for (int32_t i = 0; i < count; ++i) {
        const float* r = v + 21 * i;
        float* g = o + 25 * i;
        gpd_ctbr_outer_vjp(&b, r[0], r[1], r[2], r[3], r[4], r[5], r[6], r[7], r[8], r[9], r[10], r[11], r[12], r[13], r[14], r[15], r + 16,
                           g, g + 3, g + 7, g + 10, g + 13, g + 16);
        float again[16];
        gpd_ctbr_outer_vjp(&b, r[0], r[1], r[2], r[3], r[4], r[5], r[6], r[7], r[8], r[9], r[10], r[11], r[12], r[13], r[14], r[15], r + 16,
                           again, again + 3, again + 7, again + 10, again + 13, NULL);
        if (memcmp(again, g, sizeof again) != 0) bad |= 2;
        if (r[20] != 1.0f) continue;
        float lo[16], hi[16], clo[4], chi[4];
        double u[16], lhs = 0.0, rhs = 0.0, mag = 0.0;
        for (int k = 0; k < 16; ++k) { u[k] = 0.25 * (2.0 * draw(&seed) - 1.0); lo[k] = (float)(r[k] - STEP * u[k]); hi[k] = (float)(r[k] + STEP * u[k]); }
        gpd_ctbr_outer(&b, lo[0], lo[1], lo[2], lo[3], lo[4], lo[5], lo[6], lo[7], lo[8], lo[9], lo[10], lo[11], lo[12], lo[13], lo[14], lo[15], clo);
        gpd_ctbr_outer(&b, hi[0], hi[1], hi[2], hi[3], hi[4], hi[5], hi[6], hi[7], hi[8], hi[9], hi[10], hi[11], hi[12], hi[13], hi[14], hi[15], chi);
        for (int k = 0; k < 4; ++k) { const double ju = ((double)chi[k] - (double)clo[k]) / (2.0 * STEP); lhs += r[16 + k] * ju; mag += fabs(r[16 + k] * ju); }
        for (int k = 0; k < 16; ++k) rhs += (double)g[k] * u[k];
        const double miss = fabs(lhs - rhs) / (mag + 1e-300);
        if (miss > worst) worst = miss;
        ++checked;
    }
    printf("outer loop: <v, J u> against <J^T v, u> on %d plain rows of %d, worst mismatch %.3g of sum |v_i (J u)_i| (bound %.3g)\n", checked, count, worst, TRANSPOSE_TOL);
    if (!(worst <= TRANSPOSE_TOL) || checked < count / 8) bad |= 4;
    const int rc = write_block(out, o, count, 25);
    free(v);
    free(o);
    return rc | bad;
}

int main(int argc, char** argv) {
    if (argc == 4 && strcmp(argv[1], "rate") == 0) return write_rate(argv[2], argv[3]);
    if (argc == 4 && strcmp(argv[1], "outer") == 0) return write_outer(argv[2], argv[3]);
    defaults();

    /* ---- the tape's size ---- */
    { int64_t floats = 0; CHECK(gpd_rollout_tape_ctbr_floats(&C, 8, 128, &floats) == 0 && floats == 13 * 8 * 128, "gpd_rollout_tape_ctbr_floats: 13 K ld"); }
    { int64_t floats = 0; const int n0 = hipstub_launches(); CHECK(refused(gpd_rollout_tape_ctbr_floats(NULL, 8, 128, &floats), GPD_EINVAL, "gpd_rollout_tape_ctbr_floats", "NULL", n0), "NULL cfg"); }
    { const int n0 = hipstub_launches(); CHECK(refused(gpd_rollout_tape_ctbr_floats(&C, 8, 128, NULL), GPD_EINVAL, "gpd_rollout_tape_ctbr_floats", "NULL", n0), "NULL floats_out"); }

    /* ---- accepted: one launch of the variant mode, the plant table and g_gains select ---- */
    LAUNCHES(0, "gpd_rollout_tape_ctbr_kernel", "ILi0ELb0EE", "tape: CMD -> <CMD, no PLANT>");
    mode = GPD_CTBR_POS; rstride = 0; cmd_out = DEV(6);
    LAUNCHES(0, "gpd_rollout_tape_ctbr_kernel", "ILi1ELb0EE", "tape: POS, a held target, cmd_out -> <POS, no PLANT>");
    plant = DEV(7); ostride = 0; C.act_type = GPD_ACT_RAW_RPM; C.substeps = 1;
    LAUNCHES(0, "gpd_rollout_tape_ctbr_kernel", "ILi0ELb1EE", "tape: CMD, a plant table, last rows only, RAW_RPM -> <CMD, PLANT>");
    LAUNCHES(1, "gpd_rollout_vjp_ctbr_kernel", "ILi0ELb0ELb0EE", "sweep: CMD -> <CMD, no PLANT, no GG>");
    g_gains = DEV(14); g_obs = NULL; rstride = 0;
    LAUNCHES(1, "gpd_rollout_vjp_ctbr_kernel", "ILi0ELb0ELb1EE", "sweep: CMD, held rows, no g_obs12, g_gains -> <CMD, no PLANT, GG>");
    mode = GPD_CTBR_POS; rstride = 70 * 12; plant = DEV(7);
    LAUNCHES(1, "gpd_rollout_vjp_ctbr_kernel", "ILi1ELb1ELb0EE", "sweep: POS, a plant table -> <POS, PLANT, no GG>");
    mode = GPD_CTBR_POS; rstride = 70 * 12; g_gains = DEV(14);
    LAUNCHES(1, "gpd_rollout_vjp_ctbr_kernel", "ILi1ELb0ELb1EE", "sweep: POS, g_gains -> <POS, no PLANT, GG>");

    /* ---- GPD_ENOTSUP: where gpd_rollout_ctbr answers it, and every physics flag ---- */
    C.drones_per_env = 2; C.num_envs = 35; all_refuse(3, GPD_ENOTSUP, "drones_per_env", "aviaries of two");
    C.task = GPD_TASK_HOVER; all_refuse(3, GPD_ENOTSUP, "GPD_TASK_NONE", "a task");
    C.auto_reset = 1; all_refuse(3, GPD_ENOTSUP, "auto_reset", "auto_reset");
    for (int act = GPD_ACT_RPM; act <= GPD_ACT_DIRECT_RPM; ++act) {
        if (act == GPD_ACT_RAW_RPM || act == GPD_ACT_DIRECT_RPM) continue;
        C.act_type = act; all_refuse(3, GPD_ENOTSUP, "act_type", "another action type");
    }
    for (unsigned flag = 1; flag <= 16; flag <<= 1) { C.physics_flags = flag; all_refuse(3, GPD_ENOTSUP, "physics_flags", "a physics flag"); }
    S.dw_force = DEV(9); ONE_REFUSES(0, GPD_ENOTSUP, "dw_force", "tape: state.dw_force");
    C.num_envs = (1 << 26) + 1; S.ld = ld = (1 << 26) + 64; all_refuse(3, GPD_ERANGE, "2^26", "more than 2^26 drones");

    /* ---- GPD_EINVAL ---- */
    C.physics_flags = 32; all_refuse(3, GPD_EINVAL, "unknown physics flag", "an unknown physics flag");
    K = 0; all_refuse(3, GPD_EINVAL, "num_steps", "num_steps 0");
    C.substeps = 0; all_refuse(3, GPD_EINVAL, "positive", "substeps 0");
    S.ld = ld = 69; all_refuse(3, GPD_EINVAL, "ld", "ld < num_envs");
    mode = 2; all_refuse(2, GPD_EINVAL, "mode", "mode 2");
    rstride = -4; all_refuse(2, GPD_EINVAL, "non-negative", "a negative row stride");
    rstride = 69 * 4; all_refuse(2, GPD_EINVAL, "stride", "CMD: a row stride below 4*num_envs");
    mode = GPD_CTBR_POS; all_refuse(2, GPD_EINVAL, "stride", "POS: a row stride below 12*num_envs");
    ostride = 70 * 4; all_refuse(2, GPD_EINVAL, "stride", "an obs stride below 12*num_envs");
    rstride = 70 * 4 + 2; all_refuse(2, GPD_EINVAL, "multiples of 4", "a row stride that is no multiple of 4");
    rows = NULL; all_refuse(2, GPD_EINVAL, "NULL rows", "NULL rows");
    rows = ODD(DEV(4), 4); all_refuse(2, GPD_EINVAL, "aligned", "misaligned rows");
    plant = ODD(DEV(7), 8); all_refuse(2, GPD_EINVAL, "aligned", "misaligned plant_rows");
    obs = NULL; ONE_REFUSES(0, GPD_EINVAL, "NULL rows/obs12/tape", "tape: NULL obs12");
    tape = NULL; ONE_REFUSES(0, GPD_EINVAL, "NULL rows/obs12/tape", "tape: NULL tape");
    tape = ODD(DEV(10), 4); ONE_REFUSES(0, GPD_EINVAL, "aligned", "tape: misaligned tape");
    cmd_out = (float*)DEV(4); ONE_REFUSES(0, GPD_EINVAL, "alias", "tape: cmd_out == rows");
    S.kin = NULL; ONE_REFUSES(0, GPD_EINVAL, "NULL state.kin", "tape: NULL state.kin");
    C.pyb_dt = 0.0f; ONE_REFUSES(0, GPD_EINVAL, "positive", "tape: pyb_dt 0");
    tape_in = NULL; ONE_REFUSES(1, GPD_EINVAL, "NULL rows/tape/g_kin/g_rows", "sweep: NULL tape");
    g_kin = NULL; ONE_REFUSES(1, GPD_EINVAL, "NULL rows/tape/g_kin/g_rows", "sweep: NULL g_kin");
    g_rows = NULL; ONE_REFUSES(1, GPD_EINVAL, "NULL rows/tape/g_kin/g_rows", "sweep: NULL g_rows");
    g_kin = ODD(DEV(12), 4); ONE_REFUSES(1, GPD_EINVAL, "aligned", "sweep: misaligned g_kin");
    g_rows = ODD(DEV(13), 8); ONE_REFUSES(1, GPD_EINVAL, "aligned", "sweep: misaligned g_rows");
    g_gains = ODD(DEV(14), 4); ONE_REFUSES(1, GPD_EINVAL, "aligned", "sweep: misaligned g_gains");
    g_obs = ODD(DEV(11), 4); ONE_REFUSES(1, GPD_EINVAL, "aligned", "sweep: misaligned g_obs12");
    g_rows = (float*)DEV(12); ONE_REFUSES(1, GPD_EINVAL, "alias", "sweep: g_rows == g_kin");
    g_gains = (float*)DEV(12) + 64; ONE_REFUSES(1, GPD_EINVAL, "alias", "sweep: g_gains inside g_kin");
    g_kin = (float*)DEV(10) + 13 * 128 * 4; ONE_REFUSES(1, GPD_EINVAL, "alias", "sweep: g_kin inside the tape");
    g_gains = (float*)DEV(13) + 16; ONE_REFUSES(1, GPD_EINVAL, "alias", "sweep: g_gains inside g_rows");

    /* ---- ctbr_vjp.inc: documented corner values ---- */
    {
        GpdCtbr b;
        memset(&b, 0, sizeof b);
        b.k_rate[0] = b.k_rate[1] = 40.0f; b.k_rate[2] = 20.0f; b.thrust_max = 40.9f; b.rate_max = 6.2831855f; b.f_max = 0.15f; b.inv_kf = 1.0f / 3.16e-10f;
        const float ag[4] = {1.0f, 2.0f, 3.0f, 4.0f}, hover[4] = {9.8f, 0, 0, 0}, below[4] = {-5.0f, 0, 0, 0}, beyond[4] = {1e9f, 0, 0, 0};
        float a[4] = {0}, w[3] = {0};
        gpd_ctbr_rate_loop_vjp(&b, 0.027f, 1.4e-5f, 1.4e-5f, 2.17e-5f, 3.16e-10f, hover, 0, 0, 0, ag, a, w, NULL);
        CHECK(fabsf(a[0] - 0.25f * 0.027f * 10.0f) < 1e-7f && a[1] == 0.0f && w[0] == 0.0f, "hover, alloc 0: the thrust's cotangent is (M/4) sum ag, KF_plant inv_kf = 1");
        a[0] = 0.0f;
        gpd_ctbr_rate_loop_vjp(&b, 0.027f, 1.4e-5f, 1.4e-5f, 2.17e-5f, 3.16e-10f, below, 0, 0, 0, ag, a, w, NULL);
        CHECK(a[0] == 0.0f && a[1] == 0.0f && a[2] == 0.0f && a[3] == 0.0f && w[0] == 0.0f && w[1] == 0.0f && w[2] == 0.0f, "a negative thrust command, rotors at 0: exact zeros, finite");
        gpd_ctbr_rate_loop_vjp(&b, 0.027f, 1.4e-5f, 1.4e-5f, 2.17e-5f, 3.16e-10f, beyond, 0, 0, 0, ag, a, w, NULL);
        CHECK(a[0] == 0.0f && a[3] == 0.0f && w[2] == 0.0f, "a thrust command beyond thrust_max, rotors at f_max: exact zeros");
    }
    printf("%d checks failed\n", failed);
    return failed;
}
