/*
 * Drives the HOST side of gpd_sizeof_ctbr / gpd_ctbr / gpd_rollout_ctbr (include/gpd.h) under AddressSanitizer +
 * UndefinedBehaviorSanitizer on a machine without a GPU, the way tests/c/mppi_host.c drives gpd_mppi: libgpd's units compiled host-only
 * with the sanitizers, the HIP runtime replaced by tests/stubs/hip_stub.c (launches are counted and named, nothing runs).  Accepted
 * arguments: one launch, its geometry, and WHICH kernel (gpd_rollout_ctbr_kernel<MODE, EXT, PLANT>).  Rejected arguments: the code, a
 * message that names the entry and the reason, and no launch.  Device pointers are fake non-null addresses.
 * It also evaluates csrc/ctbr_math.inc -- the text the device kernels compile -- in fp32:
 *   ctbr_host outer IN OUT   IN: int32 count, a GpdCtbr, then count x 16 floats (pos 3 | quat xyzw 4 | vel 3 | target pos 3 | target vel 3);
 *                            OUT: count x 4 floats, the commands of gpd_ctbr_outer
 *   ctbr_host rate IN OUT    IN: int32 count, a GpdCtbr, M Jx Jy Jz, then count x 7 floats (command 4 | body rates 3);
 *                            OUT: count x 4 floats, the RPMs of gpd_ctbr_rate_loop
 * Prints one line per check; exit code = failed checks.
 */
#include <stdlib.h>

#include "host_check.h"
#include "ctbr_math.inc"

static GpdParams P;
static GpdCtbr B;
static GpdState S;
static GpdStepCfg C;
static const float *rows, *plant;
static float *obs, *cmd_out;
static int32_t mode, K;
static int64_t rstride, ostride;

static void defaults(void) {
    memset(&P, 0, sizeof P);
    memset(&B, 0, sizeof B);
    memset(&S, 0, sizeof S);
    memset(&C, 0, sizeof C);
    S.kin = DEV(1); S.step_counter = DEV(2); S.last_rpm = DEV(3); S.ld = 128;
    C.num_envs = 70; C.drones_per_env = 1; C.act_type = GPD_ACT_DIRECT_RPM; C.substeps = 5; C.pyb_dt = 1.0f / 240; C.ctrl_dt = 1.0f / 48;
    C.inv_ctrl_dt = 48.0f; C.lanes_per_wave = 64; C.task = GPD_TASK_NONE;
    rows = DEV(4); plant = NULL; obs = DEV(5); cmd_out = NULL;
    mode = GPD_CTBR_CMD; K = 24; rstride = 0; ostride = 70 * 12;
}
static int call(void) { return gpd_rollout_ctbr(&P, &B, &S, &C, mode, rows, rstride, plant, obs, ostride, cmd_out, K, NULL); }
#define REFUSED(code, reason, what) do { const int n0_ = hipstub_launches(); CHECK(refused(call(), code, "gpd_rollout_ctbr", reason, n0_), what); defaults(); } while (0)
#define LAUNCHES(piece, what) do { const int n0_ = hipstub_launches(); unsigned g_[7]; const int rc_ = call(); hipstub_last(g_); \
    CHECK(rc_ == 0 && hipstub_launches() == n0_ + 1 && KERNEL("gpd_rollout_ctbr_kernel") && KERNEL(piece) && g_[0] == 1 && g_[3] == 256, what); defaults(); } while (0)

static float* read_block(const char* path, int32_t* count, GpdCtbr* b, float* extra, int n_extra, int width) {
    FILE* f = fopen(path, "rb");
    if (!f || fread(count, 4, 1, f) != 1 || *count < 0 || fread(b, sizeof *b, 1, f) != 1) return NULL;
    if (n_extra && fread(extra, 4, (size_t)n_extra, f) != (size_t)n_extra) return NULL;
    float* v = malloc((size_t)*count * (size_t)width * 4 + 4);
    if (!v || fread(v, (size_t)width * 4, (size_t)*count, f) != (size_t)*count) return NULL;
    fclose(f);
    return v;
}
static int write_block(const char* path, const float* o, int32_t count) {
    FILE* f = fopen(path, "wb");
    if (!f || fwrite(o, 16, (size_t)count, f) != (size_t)count) return 1;
    return fclose(f) != 0;
}

static int write_outer(const char* in, const char* out) {
    int32_t count = 0;
    GpdCtbr b;
    float* v = read_block(in, &count, &b, NULL, 0, 16);
    float* o = malloc((size_t)count * 16 + 4);
    if (!v || !o) return 1;
    for (int32_t i = 0; i < count; ++i) {
        const float* r = v + 16 * i;
        gpd_ctbr_outer(&b, r[0], r[1], r[2], r[3], r[4], r[5], r[6], r[7], r[8], r[9], r[10], r[11], r[12], r[13], r[14], r[15], o + 4 * i);
    }
    const int rc = write_block(out, o, count);
    free(v);
    free(o);
    return rc;
}

static int write_rate(const char* in, const char* out) {
    int32_t count = 0;
    GpdCtbr b;
    float mj[4];
    float* v = read_block(in, &count, &b, mj, 4, 7);
    float* o = malloc((size_t)count * 16 + 4);
    if (!v || !o) return 1;
    for (int32_t i = 0; i < count; ++i) gpd_ctbr_rate_loop(&b, mj[0], mj[1], mj[2], mj[3], v + 7 * i, v[7 * i + 4], v[7 * i + 5], v[7 * i + 6], o + 4 * i);
    const int rc = write_block(out, o, count);
    free(v);
    free(o);
    return rc;
}

int main(int argc, char** argv) {
    if (argc == 4 && strcmp(argv[1], "outer") == 0) return write_outer(argv[2], argv[3]);
    if (argc == 4 && strcmp(argv[1], "rate") == 0) return write_rate(argv[2], argv[3]);
    defaults();

    /* ---- gpd_sizeof_ctbr ---- */
    { int32_t size = 0; CHECK(gpd_sizeof_ctbr(&size) == 0 && size == (int32_t)sizeof(GpdCtbr) && size % 16 == 0 && size == 128, "gpd_sizeof_ctbr: 128 bytes"); }
    { const int n0 = hipstub_launches(); CHECK(refused(gpd_sizeof_ctbr(NULL), GPD_EINVAL, "gpd_sizeof_ctbr", "NULL", n0), "gpd_sizeof_ctbr(NULL)"); }

    /* ---- gpd_ctbr ---- */
    {
        unsigned g[7];
        int n0 = hipstub_launches();
        int rc = gpd_ctbr(&B, DEV(1), DEV(2), DEV(3), DEV(4), DEV(5), DEV(6), 70, NULL);
        hipstub_last(g);
        CHECK(rc == 0 && hipstub_launches() == n0 + 1 && KERNEL("gpd_ctbr_kernel") && g[0] == 1 && g[3] == 256, "gpd_ctbr: 70 drones, one workgroup");
        n0 = hipstub_launches();
        rc = gpd_ctbr(&B, DEV(1), DEV(2), DEV(3), DEV(4), NULL, DEV(6), 257, NULL);
        hipstub_last(g);
        CHECK(rc == 0 && hipstub_launches() == n0 + 1 && g[0] == 2, "gpd_ctbr: no target velocity, 257 drones in two workgroups");
#define CTBR_REFUSED(expr, code, reason, what) do { const int n0_ = hipstub_launches(); CHECK(refused(expr, code, "gpd_ctbr", reason, n0_), what); } while (0)
        CTBR_REFUSED(gpd_ctbr(NULL, DEV(1), DEV(2), DEV(3), DEV(4), DEV(5), DEV(6), 70, NULL), GPD_EINVAL, "NULL", "NULL ctbr");
        CTBR_REFUSED(gpd_ctbr(&B, NULL, DEV(2), DEV(3), DEV(4), DEV(5), DEV(6), 70, NULL), GPD_EINVAL, "NULL", "NULL cur_pos");
        CTBR_REFUSED(gpd_ctbr(&B, DEV(1), NULL, DEV(3), DEV(4), DEV(5), DEV(6), 70, NULL), GPD_EINVAL, "NULL", "NULL cur_quat");
        CTBR_REFUSED(gpd_ctbr(&B, DEV(1), DEV(2), NULL, DEV(4), DEV(5), DEV(6), 70, NULL), GPD_EINVAL, "NULL", "NULL cur_vel");
        CTBR_REFUSED(gpd_ctbr(&B, DEV(1), DEV(2), DEV(3), NULL, DEV(5), DEV(6), 70, NULL), GPD_EINVAL, "NULL", "NULL target_pos");
        CTBR_REFUSED(gpd_ctbr(&B, DEV(1), DEV(2), DEV(3), DEV(4), DEV(5), NULL, 70, NULL), GPD_EINVAL, "NULL", "NULL cmd");
        CTBR_REFUSED(gpd_ctbr(&B, DEV(1), DEV(2), DEV(3), DEV(4), DEV(5), DEV(6), 0, NULL), GPD_EINVAL, "positive", "n 0");
        CTBR_REFUSED(gpd_ctbr(&B, DEV(1), DEV(2), DEV(3), DEV(4), DEV(5), DEV(6), -3, NULL), GPD_EINVAL, "positive", "n negative");
        CTBR_REFUSED(gpd_ctbr(&B, DEV(1), DEV(2), DEV(3), DEV(4), DEV(5), DEV(6), (1 << 26) + 1, NULL), GPD_ERANGE, "2^26", "n above 2^26");
        CTBR_REFUSED(gpd_ctbr(&B, DEV(1), ODD(DEV(2), 4), DEV(3), DEV(4), DEV(5), DEV(6), 70, NULL), GPD_EINVAL, "aligned", "misaligned cur_quat");
        CTBR_REFUSED(gpd_ctbr(&B, DEV(1), DEV(2), DEV(3), DEV(4), DEV(5), ODD(DEV(6), 8), 70, NULL), GPD_EINVAL, "aligned", "misaligned cmd");
    }

    /* ---- gpd_rollout_ctbr, accepted: one launch of the variant mode, flags and the plant table select ---- */
    LAUNCHES("ILi0ELb0ELb0E", "CMD, held commands -> <CMD, no EXT, no PLANT>");
    rstride = 70 * 4; cmd_out = DEV(6);
    LAUNCHES("ILi0ELb0ELb0E", "CMD, a block per step, cmd_out -> <CMD, no EXT, no PLANT>");
    mode = GPD_CTBR_POS;
    LAUNCHES("ILi1ELb0ELb0E", "POS, a held target -> <POS, no EXT, no PLANT>");
    mode = GPD_CTBR_POS; rstride = 70 * 12; C.physics_flags = GPD_PHYS_DRAG | GPD_PHYS_GND; C.act_type = GPD_ACT_RAW_RPM; C.substeps = 8;
    LAUNCHES("ILi1ELb1ELb0E", "POS, targets per step, drag and ground effect, RAW_RPM -> <POS, EXT, no PLANT>");
    plant = DEV(7); C.physics_flags = GPD_PHYS_GROUND | GPD_PHYS_DAMP; ostride = 0; C.substeps = 1;
    LAUNCHES("ILi0ELb1ELb1E", "CMD, a plant table, ground plane and damping, last rows only, one sub-step -> <CMD, EXT, PLANT>");
    mode = GPD_CTBR_POS; plant = DEV(7); S.last_rpm = NULL; S.bad = DEV(8);
    LAUNCHES("ILi1ELb0ELb1E", "POS, a plant table, no last_rpm (no drag), a guard -> <POS, no EXT, PLANT>");

    /* ---- GPD_EINVAL ---- */
    { const int n0 = hipstub_launches(); CHECK(refused(gpd_rollout_ctbr(NULL, &B, &S, &C, mode, rows, 0, NULL, obs, ostride, NULL, K, NULL), GPD_EINVAL, "gpd_rollout_ctbr", "NULL", n0), "NULL params"); }
    { const int n0 = hipstub_launches(); CHECK(refused(gpd_rollout_ctbr(&P, NULL, &S, &C, mode, rows, 0, NULL, obs, ostride, NULL, K, NULL), GPD_EINVAL, "gpd_rollout_ctbr", "NULL", n0), "NULL ctbr"); }
    { const int n0 = hipstub_launches(); CHECK(refused(gpd_rollout_ctbr(&P, &B, NULL, &C, mode, rows, 0, NULL, obs, ostride, NULL, K, NULL), GPD_EINVAL, "gpd_rollout_ctbr", "NULL", n0), "NULL state"); }
    { const int n0 = hipstub_launches(); CHECK(refused(gpd_rollout_ctbr(&P, &B, &S, NULL, mode, rows, 0, NULL, obs, ostride, NULL, K, NULL), GPD_EINVAL, "gpd_rollout_ctbr", "NULL", n0), "NULL cfg"); }
    S.kin = NULL; REFUSED(GPD_EINVAL, "NULL state.kin", "NULL state.kin");
    S.step_counter = NULL; REFUSED(GPD_EINVAL, "NULL state.kin", "NULL state.step_counter");
    rows = NULL; REFUSED(GPD_EINVAL, "NULL rows/obs12", "NULL rows");
    obs = NULL; REFUSED(GPD_EINVAL, "NULL rows/obs12", "NULL obs12");
    S.kin = ODD(DEV(1), 4); REFUSED(GPD_EINVAL, "16-byte", "misaligned state.kin");
    mode = 2; REFUSED(GPD_EINVAL, "mode", "mode 2");
    mode = -1; REFUSED(GPD_EINVAL, "mode", "mode -1");
    K = 0; REFUSED(GPD_EINVAL, "num_steps", "num_steps 0");
    rstride = -4; REFUSED(GPD_EINVAL, "non-negative", "negative row stride");
    ostride = -12; REFUSED(GPD_EINVAL, "non-negative", "negative obs stride");
    C.physics_flags = 32; REFUSED(GPD_EINVAL, "unknown physics flag", "an unknown physics flag");
    C.num_envs = 0; REFUSED(GPD_EINVAL, "positive", "num_envs 0");
    C.substeps = 0; REFUSED(GPD_EINVAL, "positive", "substeps 0");
    S.ld = 69; REFUSED(GPD_EINVAL, "state.ld", "state.ld < num_envs");
    C.physics_flags = GPD_PHYS_DRAG; S.last_rpm = NULL; REFUSED(GPD_EINVAL, "GPD_PHYS_DRAG needs state.last_rpm", "drag without last_rpm");
    rstride = 69 * 4; REFUSED(GPD_EINVAL, "stride", "CMD: a row stride below 4*num_envs");
    mode = GPD_CTBR_POS; rstride = 70 * 4; REFUSED(GPD_EINVAL, "stride", "POS: a row stride below 12*num_envs");
    ostride = 70 * 4; REFUSED(GPD_EINVAL, "stride", "an obs stride below 12*num_envs");
    rstride = 70 * 4 + 2; REFUSED(GPD_EINVAL, "multiples of 4", "a row stride that is no multiple of 4");
    ostride = 70 * 12 + 1; REFUSED(GPD_EINVAL, "multiples of 4", "an obs stride that is no multiple of 4");
    rows = ODD(DEV(4), 4); REFUSED(GPD_EINVAL, "aligned", "misaligned rows");
    obs = ODD(DEV(5), 8); REFUSED(GPD_EINVAL, "aligned", "misaligned obs12");
    plant = ODD(DEV(7), 12); REFUSED(GPD_EINVAL, "aligned", "misaligned plant_rows");
    cmd_out = ODD(DEV(6), 4); REFUSED(GPD_EINVAL, "aligned", "misaligned cmd_out");
    cmd_out = (float*)DEV(4); REFUSED(GPD_EINVAL, "alias", "cmd_out == rows");
    C.ctrl_dt = 0.0f; REFUSED(GPD_EINVAL, "positive", "ctrl_dt 0");
    C.pyb_dt = -1.0f; REFUSED(GPD_EINVAL, "positive", "pyb_dt negative");

    /* ---- GPD_ENOTSUP: what the kernel does not serve ---- */
    C.drones_per_env = 2; C.num_envs = 35; REFUSED(GPD_ENOTSUP, "one drone", "aviaries of two");
    C.task = GPD_TASK_HOVER; REFUSED(GPD_ENOTSUP, "GPD_TASK_NONE", "a task");
    C.auto_reset = 1; REFUSED(GPD_ENOTSUP, "GPD_TASK_NONE", "auto_reset");
    for (int act = GPD_ACT_RPM; act <= GPD_ACT_DIRECT_RPM; ++act) {
        if (act == GPD_ACT_RAW_RPM || act == GPD_ACT_DIRECT_RPM) continue;
        C.act_type = act; REFUSED(GPD_ENOTSUP, "act_type", "another action type");
    }
    C.physics_flags = GPD_PHYS_DW; REFUSED(GPD_ENOTSUP, "downwash", "GPD_PHYS_DW");
    S.dw_force = DEV(9); REFUSED(GPD_ENOTSUP, "downwash", "state.dw_force");
    C.num_envs = (1 << 26) + 1; S.ld = (1 << 26) + 64; REFUSED(GPD_ERANGE, "2^26", "more than 2^26 drones");

    /* ---- ctbr_math.inc: documented corner values ---- */
    {
        GpdCtbr b;
        memset(&b, 0, sizeof b);
        b.k_p[0] = b.k_p[1] = 3.0f; b.k_p[2] = 8.0f; b.k_d[0] = b.k_d[1] = 2.5f; b.k_d[2] = 5.0f; b.k_rates[0] = b.k_rates[1] = 5.0f; b.k_rates[2] = 1.0f; b.g = 9.8f;
        b.k_rate[0] = b.k_rate[1] = 40.0f; b.k_rate[2] = 20.0f; b.thrust_max = 40.9f; b.rate_max = 6.2831855f; b.f_max = 0.15f; b.inv_kf = 1.0f / 3.16e-10f;
        float c[4], rpm[4];
        gpd_ctbr_outer(&b, 0, 0, 1, 0, 0, 0, 1, 0, 0, 0, 0, 0, 1, 0, 0, 0, c);
        CHECK(c[0] == 9.8f && c[1] == 0.0f && c[2] == 0.0f && c[3] == 0.0f, "level at the target: thrust g, no rates");
        gpd_ctbr_outer(&b, 0, 0, 1, 0, 0, 0, -1, 0, 0, 0, 0, 0, 1, 0, 0, 0, c);
        CHECK(c[0] == 9.8f && c[1] == 0.0f && c[2] == 0.0f && c[3] == 0.0f, "... and with the quaternion's other sign");
        const float hover[4] = {9.8f, 0, 0, 0}, beyond[4] = {1e9f, -1e9f, 1e9f, 1e9f}, below[4] = {-5.0f, 0, 0, 0};
        gpd_ctbr_rate_loop(&b, 0.027f, 1.4e-5f, 1.4e-5f, 2.17e-5f, hover, 0, 0, 0, rpm);
        CHECK(rpm[0] == rpm[1] && rpm[1] == rpm[2] && rpm[2] == rpm[3] && rpm[0] > 14400.0f && rpm[0] < 14500.0f, "hover command, no rates: four equal RPMs (alloc 0 here)");
        gpd_ctbr_rate_loop(&b, 0.027f, 1.4e-5f, 1.4e-5f, 2.17e-5f, beyond, 0, 0, 0, rpm);
        CHECK(rpm[0] == rpm[3] && rpm[0] == sqrtf(b.f_max * b.inv_kf), "a command beyond the clips: thrust_max, rotors at f_max");
        gpd_ctbr_rate_loop(&b, 0.027f, 1.4e-5f, 1.4e-5f, 2.17e-5f, below, 0, 0, 0, rpm);
        CHECK(rpm[0] == 0.0f && rpm[3] == 0.0f, "a negative thrust command: 0 RPM");
    }
    printf("%d checks failed\n", failed);
    return failed;
}
