/*
 * Drives the HOST side of the three entries of the differentiable rollout through the DSLPID loop (include/gpd.h:
 * gpd_rollout_tape_pid_floats, gpd_rollout_tape_pid, gpd_rollout_vjp_pid) under AddressSanitizer + UndefinedBehaviorSanitizer on a
 * machine without a GPU, the way tests/c/diff_host.c drives the RPM entries: libgpd's five units compiled host-only with the sanitizers,
 * the HIP runtime replaced by tests/stubs/hip_stub.c (launches are counted and named, nothing runs).  Accepted arguments: the tape's
 * size, one launch each, its geometry, and WHICH kernel (gpd_rollout_tape_pid_kernel<AW>, gpd_rollout_vjp_pid_kernel<AW, GG>: GG 1 with
 * g_gains, GG 0 without).  Rejected arguments: the code, a message that names the entry and the reason, and no launch.  Device pointers
 * are fake non-null addresses: host code must never dereference them.
 * With a file name as its argument it also evaluates csrc/dslpid_vjp.inc -- the text the device sweep compiles -- on controller inputs
 * it draws itself and writes inputs and outputs there, one call per line, for tests/test_host_diff_pid.py to hold against float64
 * autograd of the restatement's controller.
 * Prints one line per check; exit code = failed checks.
 */
#define _GNU_SOURCE
#include <math.h>

#include "host_check.h"
#include "dslpid_vjp.inc"

static GpdParams P;
static GpdState S;
static GpdStepCfg C;

static int tape_call(int K) {
    return gpd_rollout_tape_pid(&P, &S, &C, K, DEV(3), 4096 * 4, DEV(4), DEV(6), 4096 * 12, DEV(7), DEV(8), DEV(9), 4096, DEV(12), NULL);
}
static int vjp_gains_call(int K, float* g_gains) {
    return gpd_rollout_vjp_pid(&P, &C, S.ld, K, DEV(3), 4096 * 4, DEV(4), DEV(12), DEV(13), 4096 * 12, DEV(14), 4096, DEV(15), DEV(18), DEV(16),
                               g_gains, NULL);
}
static int vjp_call(int K) { return vjp_gains_call(K, DEV(19)); }
static int floats_call(int K) { int64_t floats; return gpd_rollout_tape_pid_floats(&C, K, S.ld, &floats); }

static const struct { const char* name; int (*call)(int K); } ENTRIES[3] = {
    {"gpd_rollout_tape_pid", tape_call}, {"gpd_rollout_vjp_pid", vjp_call}, {"gpd_rollout_tape_pid_floats", floats_call}};
/* the first `entries` of them refuse the configuration as it stands: the code, the entry and the reason, nothing launched */
static void all_refuse(int entries, int K, int code, const char* reason, const char* what, int n0) {
    char line[160];
    for (int e = 0; e < entries; ++e) {
        snprintf(line, sizeof line, "%s: %s", ENTRIES[e].name, what);
        CHECK(refused(ENTRIES[e].call(K), code, ENTRIES[e].name, reason, n0), line);
    }
}

/* the CF2X controller (control/DSLPIDControl.py:37-60), as params.py packs it */
static void cf2x_controller(GpdParams* p) {
    const float gains[6][3] = {{.4f, .4f, 1.25f}, {.05f, .05f, .05f}, {.2f, .2f, .5f}, {70000.f, 70000.f, 60000.f}, {.0f, .0f, 500.f}, {20000.f, 20000.f, 12000.f}};
    const float mixer[12] = {-.5f, -.5f, -1, -.5f, .5f, 1, .5f, .5f, -1, .5f, -.5f, 1};
    for (int k = 0; k < 3; ++k) {
        p->p_for[k] = gains[0][k]; p->i_for[k] = gains[1][k]; p->d_for[k] = gains[2][k];
        p->p_tor[k] = gains[3][k]; p->i_tor[k] = gains[4][k]; p->d_tor[k] = gains[5][k];
    }
    for (int k = 0; k < 12; ++k) p->mixer[k] = mixer[k];
    p->pid_gravity = (float)(9.8 * 0.027); p->pid_kf = 3.16e-10f; p->pid_inv_4kf = (float)(1.0 / (4.0 * 3.16e-10));
    p->pwm2rpm_scale = 0.2685f; p->inv_pwm2rpm_scale = (float)(1.0 / 0.2685); p->pwm2rpm_const = 4070.3f; p->min_pwm = 20000.f; p->max_pwm = 65535.f;
    p->KF = 3.16e-10f; p->speed_limit = 0.25f;
}

static double draw(uint64_t* x) { *x = *x * 6364136223846793005ull + 1442695040888963407ull; return (double)(*x >> 11) / 9007199254740992.0; }
static float sym(uint64_t* x, double half) { return (float)(half * (2.0 * draw(x) - 1.0)); }

/* dslpid_vjp.inc on the host: 400 calls around hover -- position errors of a few decimetres, tilts of a few hundredths of a radian, a
 * last rpy within 2e-3 rad, members on both sides of their clamps -- so that every clamp of the controller is met engaged and free */
static int write_formulas(const char* path) {
    GpdParams N;
    memset(&N, 0, sizeof N);
    cf2x_controller(&N);
    const float dt = 1.0f / 48, inv_dt = 48.0f;
    FILE* f = fopen(path, "w");
    if (!f) return 1;
    fprintf(f, "%.9g %.9g", dt, N.pid_gravity);
    fprintf(f, " %.9g %.9g %.9g %.9g %.9g %.9g\n", N.pid_kf, N.pwm2rpm_scale, N.pwm2rpm_const, N.min_pwm, N.max_pwm, N.pid_inv_4kf);
    uint64_t seed = 2024;
    for (int d = 0; d < 400; ++d) {
        GpdDslVars X, a;
        GpdDslOutCot o;
        GpdDslGainCot G;
        memset(&a, 0, sizeof a);
        memset(&G, 0, sizeof G);
        const double big = draw(&seed) < 0.15 ? 6.0 : 1.0;           /* now and then a drone far from its target, tilted and fast */
        X.px = sym(&seed, 0.2); X.py = sym(&seed, 0.2); X.pz = 1.0f + sym(&seed, 0.2);
        X.tx = X.px + sym(&seed, 0.3 * big); X.ty = X.py + sym(&seed, 0.3 * big); X.tz = X.pz + sym(&seed, 0.3 * big);
        X.vx = sym(&seed, 0.5); X.vy = sym(&seed, 0.5); X.vz = sym(&seed, 0.5 * big);
        X.tvx = sym(&seed, 0.25); X.tvy = sym(&seed, 0.25); X.tvz = sym(&seed, 0.25);
        X.roll = sym(&seed, 0.03 * big); X.pitch = sym(&seed, 0.03 * big); X.yaw = sym(&seed, 3.0);
        X.tyaw = draw(&seed) < 0.5 ? X.yaw : sym(&seed, 3.0);
        {   /* R of that attitude, in double (btQuaternion::setEulerZYX, btMatrix3x3::setRotation) */
            const double hr = 0.5 * X.roll, hp = 0.5 * X.pitch, hy = 0.5 * X.yaw;
            const double x = sin(hr) * cos(hp) * cos(hy) - cos(hr) * sin(hp) * sin(hy), y = cos(hr) * sin(hp) * cos(hy) + sin(hr) * cos(hp) * sin(hy);
            const double z = cos(hr) * cos(hp) * sin(hy) - sin(hr) * sin(hp) * cos(hy), w = cos(hr) * cos(hp) * cos(hy) + sin(hr) * sin(hp) * sin(hy);
            X.r00 = (float)(1 - 2 * (y * y + z * z)); X.r01 = (float)(2 * (x * y - w * z)); X.r02 = (float)(2 * (x * z + w * y));
            X.r10 = (float)(2 * (x * y + w * z)); X.r11 = (float)(1 - 2 * (x * x + z * z)); X.r12 = (float)(2 * (y * z - w * x));
            X.r20 = (float)(2 * (x * z - w * y)); X.r21 = (float)(2 * (y * z + w * x)); X.r22 = (float)(1 - 2 * (x * x + y * y));
        }
        X.lr = X.roll + sym(&seed, 2e-3); X.lp = X.pitch + sym(&seed, 2e-3); X.ly = X.yaw + sym(&seed, 2e-3);
        X.ipx = sym(&seed, 0.1) * (float)(big * big); X.ipy = sym(&seed, 0.1) * (float)(big * big); X.ipz = sym(&seed, 0.2);
        X.irx = sym(&seed, 1.2); X.iry = sym(&seed, 1.2); X.irz = sym(&seed, big > 1.0 ? 1600.0 : 2.0);
        o.rpm0 = sym(&seed, 1.0); o.rpm1 = sym(&seed, 1.0); o.rpm2 = sym(&seed, 1.0); o.rpm3 = sym(&seed, 1.0);
        o.ipx = sym(&seed, 1.0); o.ipy = sym(&seed, 1.0); o.ipz = sym(&seed, 1.0); o.lr = sym(&seed, 1.0); o.lp = sym(&seed, 1.0); o.ly = sym(&seed, 1.0);
        o.irx = sym(&seed, 1.0); o.iry = sym(&seed, 1.0); o.irz = sym(&seed, 1.0);
        gpd_dslpid_vjp(&N, dt, inv_dt, &X, &o, &a, &G);
        {   /* the flag: without the gains' cotangents the others are the same bits */
            GpdDslVars b;
            memset(&b, 0, sizeof b);
            gpd_dslpid_vjp(&N, dt, inv_dt, &X, &o, &b, NULL);
            if (memcmp(&a, &b, sizeof a) != 0) { fclose(f); return 2; }
        }
        const float* xs = (const float*)&X; const float* os = (const float*)&o; const float* as = (const float*)&a; const float* gs = (const float*)&G;
        for (size_t k = 0; k < sizeof X / sizeof(float); ++k) fprintf(f, "%.9g ", xs[k]);
        for (size_t k = 0; k < sizeof o / sizeof(float); ++k) fprintf(f, "%.9g ", os[k]);
        for (size_t k = 0; k < sizeof a / sizeof(float); ++k) fprintf(f, "%.9g ", as[k]);
        for (size_t k = 0; k < sizeof G / sizeof(float); ++k) fprintf(f, "%.9g%c", gs[k], k + 1 < sizeof G / sizeof(float) ? ' ' : '\n');
    }
    return fclose(f) != 0;
}

int main(int argc, char** argv) {
    memset(&P, 0, sizeof P);
    memset(&S, 0, sizeof S);
    memset(&C, 0, sizeof C);
    unsigned last[7];
    cf2x_controller(&P);
    S.kin = DEV(1); S.step_counter = DEV(2); S.ld = 4096; S.last_rpm = DEV(10); S.pid = DEV(11);
    C.num_envs = 4096; C.drones_per_env = 1; C.substeps = 5; C.act_type = GPD_ACT_VEL; C.task = GPD_TASK_HOVER; C.pyb_dt = 1.0f / 240;
    C.ctrl_dt = 1.0f / 48; C.inv_ctrl_dt = 48;

    /* ---- the size query ---- */
    int64_t floats = -1;
    CHECK(gpd_rollout_tape_pid_floats(&C, 20, 4096, &floats) == 0 && floats == 22 * 20 * 4096LL, "tape of 20 steps: 13 + 9 rows per step, times ld");
    C.num_envs = 70;
    CHECK(gpd_rollout_tape_pid_floats(&C, 1, 128, &floats) == 0 && floats == 22 * 128, "70 drones at ld = 128, one step");
    CHECK(gpd_rollout_tape_pid_floats(&C, 1, 64, &floats) == GPD_EINVAL, "ld below the number of drones");
    C.num_envs = 4096;
    CHECK(gpd_rollout_tape_pid_floats(NULL, 1, 4096, &floats) == GPD_EINVAL && gpd_rollout_tape_pid_floats(&C, 1, 4096, NULL) == GPD_EINVAL, "NULL cfg / floats_out");
    CHECK(gpd_rollout_tape_pid_floats(&C, 0, 4096, &floats) == GPD_EINVAL, "num_steps 0");
    CHECK(gpd_rollout_tape_pid_floats(&C, 2147483647, 0xffffffffLL, &floats) == GPD_ERANGE, "a tape beyond 2^63 floats -> GPD_ERANGE");
    CHECK(gpd_rollout_tape_pid_floats(&C, 1, 1ll << 32, &floats) == GPD_EINVAL, "a pitch beyond 2^32 - 1");

    /* ---- accepted calls: one launch each, the kernel named ---- */
    int n0 = hipstub_launches();
    CHECK(tape_call(20) == 0 && hipstub_launches() == n0 + 1, "gpd_rollout_tape_pid launches once");
    hipstub_last(last);
    CHECK(last[0] == 16 && last[3] == 256 && last[6] == 0, "4096 drones: 16 workgroups of 256 lanes, no dynamic LDS");
    CHECK(KERNEL("gpd_rollout_tape_pid_kernelILi4EE"), "VEL -> gpd_rollout_tape_pid_kernel<AW 4>");
    CHECK(vjp_call(20) == 0 && hipstub_launches() == n0 + 2, "gpd_rollout_vjp_pid launches once");
    hipstub_last(last);
    CHECK(last[0] == 16 && last[3] == 256 && last[6] == 0, "the reverse sweep: one lane per drone");
    CHECK(KERNEL("gpd_rollout_vjp_pid_kernelILi4ELb1EE"), "with g_gains -> gpd_rollout_vjp_pid_kernel<AW 4, GG 1>");
    CHECK(vjp_gains_call(20, NULL) == 0 && hipstub_launches() == n0 + 3 && KERNEL("gpd_rollout_vjp_pid_kernelILi4ELb0EE"),
          "without g_gains -> <AW 4, GG 0>, one launch");
    C.act_type = GPD_ACT_PID;
    CHECK(tape_call(3) == 0 && KERNEL("gpd_rollout_tape_pid_kernelILi3EE"), "PID -> gpd_rollout_tape_pid_kernel<AW 3>");
    CHECK(vjp_call(3) == 0 && KERNEL("gpd_rollout_vjp_pid_kernelILi3ELb1EE"), "... its sweep with g_gains -> <AW 3, GG 1>");
    CHECK(vjp_gains_call(3, NULL) == 0 && KERNEL("gpd_rollout_vjp_pid_kernelILi3ELb0EE"), "... and without -> <AW 3, GG 0>");
    C.act_type = GPD_ACT_ONE_D_PID;
    CHECK(tape_call(3) == 0 && KERNEL("gpd_rollout_tape_pid_kernelILi1EE"), "ONE_D_PID -> gpd_rollout_tape_pid_kernel<AW 1>");
    CHECK(vjp_call(3) == 0 && KERNEL("gpd_rollout_vjp_pid_kernelILi1ELb1EE"), "... its sweep with g_gains -> <AW 1, GG 1>");
    CHECK(vjp_gains_call(3, NULL) == 0 && KERNEL("gpd_rollout_vjp_pid_kernelILi1ELb0EE"), "... and without -> <AW 1, GG 0>");
    C.act_type = GPD_ACT_VEL;
    CHECK(gpd_rollout_vjp_pid(&P, &C, S.ld, 20, DEV(3), 0, DEV(4), DEV(12), NULL, 0, NULL, 0, DEV(15), DEV(18), DEV(16), NULL, NULL) == 0,
          "NULL cotangents of obs12 and reward (zeros), a shared action block");
    C.task = GPD_TASK_NONE;
    CHECK(gpd_rollout_tape_pid(&P, &S, &C, 5, DEV(3), 4096 * 4, NULL, DEV(6), 4096 * 12, DEV(7), DEV(8), DEV(9), 4096, DEV(12), NULL) == 0,
          "no task needs no target");
    CHECK(gpd_rollout_vjp_pid(&P, &C, S.ld, 5, DEV(3), 4096 * 4, NULL, DEV(12), DEV(13), 4096 * 12, NULL, 0, DEV(15), DEV(18), DEV(16), NULL, NULL) == 0,
          "... in the reverse sweep either");
    C.task = GPD_TASK_HOVER;
    S.last_rpm = NULL;
    CHECK(tape_call(2) == 0, "state.last_rpm is optional");
    S.last_rpm = DEV(10);
    C.num_envs = 70; S.ld = 128;
    CHECK(tape_call(2) == 0 && vjp_call(2) == 0, "70 drones at ld = 128");
    hipstub_last(last);
    CHECK(last[0] == 1 && last[3] == 256, "... one workgroup");
    C.num_envs = 4096; S.ld = 4096;

    /* ---- rejected configurations: GPD_ENOTSUP from every entry, nothing launched ---- */
    n0 = hipstub_launches();
    const int rpm_acts[4] = {GPD_ACT_RPM, GPD_ACT_ONE_D_RPM, GPD_ACT_RAW_RPM, GPD_ACT_DIRECT_RPM};
    for (int i = 0; i < 4; ++i) {
        C.act_type = rpm_acts[i];
        all_refuse(3, 4, GPD_ENOTSUP, "gpd_rollout_tape / gpd_rollout_vjp", "an RPM action type, pointed to the RPM entries", n0);
    }
    C.act_type = GPD_ACT_VEL;
    const uint32_t flags[6] = {GPD_PHYS_DRAG, GPD_PHYS_GND, GPD_PHYS_DW, GPD_PHYS_GROUND, GPD_PHYS_DAMP, GPD_PHYS_DRAG | GPD_PHYS_GND};
    for (int i = 0; i < 6; ++i) {
        C.physics_flags = flags[i];
        all_refuse(3, 4, GPD_ENOTSUP, "physics_flags", "a physics flag, drag included", n0);
    }
    C.physics_flags = 32;
    all_refuse(3, 4, GPD_EINVAL, "unknown physics flag", "an unknown flag", n0);
    C.physics_flags = 0;
    C.drones_per_env = 2; C.num_envs = 2048;
    all_refuse(3, 4, GPD_ENOTSUP, "drones_per_env", "aviaries of two drones", n0);
    C.drones_per_env = 1; C.num_envs = 4096;
    C.task = GPD_TASK_MULTIHOVER;
    all_refuse(3, 4, GPD_ENOTSUP, "task", "the multi-drone task", n0);
    C.task = GPD_TASK_HOVER;
    C.auto_reset = 1;
    all_refuse(3, 4, GPD_ENOTSUP, "auto_reset", "auto_reset", n0);
    C.auto_reset = 0;
    C.num_envs = (1 << 26) + 1; S.ld = (1ll << 26) + 64;
    all_refuse(3, 1, GPD_ERANGE, "2^26", "more than 2^26 drones", n0);
    C.num_envs = 4096; S.ld = 4096;
    S.dw_force = DEV(17);
    CHECK(refused(tape_call(4), GPD_ENOTSUP, "gpd_rollout_tape_pid", "dw_force", n0), "gpd_rollout_tape_pid: downwash computed outside the kernel");
    S.dw_force = NULL;
    P.pid_kf = 0.0f;
    all_refuse(2, 4, GPD_ENOTSUP, "no DSLPID controller", "an airframe without DSLPID (pid_kf <= 0)", n0);
    P.pid_kf = 3.16e-10f;

    /* ---- bad arguments: GPD_EINVAL, nothing launched ---- */
    S.pid = NULL;
    CHECK(refused(tape_call(4), GPD_EINVAL, "gpd_rollout_tape_pid", "state.pid", n0), "a missing state.pid");
    S.pid = DEV(11);
    CHECK(refused(tape_call(0), GPD_EINVAL, "gpd_rollout_tape_pid", "num_steps", n0), "K = 0");
    CHECK(refused(vjp_call(-1), GPD_EINVAL, "gpd_rollout_vjp_pid", "num_steps", n0), "K = -1");
    CHECK(refused(gpd_rollout_tape_pid(NULL, &S, &C, 4, DEV(3), 0, DEV(4), DEV(6), 0, DEV(7), DEV(8), DEV(9), 0, DEV(12), NULL), GPD_EINVAL,
                  "gpd_rollout_tape_pid", "NULL", n0), "NULL params");
    CHECK(refused(gpd_rollout_tape_pid(&P, &S, &C, 4, DEV(3), 0, DEV(4), DEV(6), 0, DEV(7), DEV(8), DEV(9), 0, NULL, NULL), GPD_EINVAL,
                  "gpd_rollout_tape_pid", "NULL", n0), "NULL tape");
    CHECK(refused(gpd_rollout_tape_pid(&P, &S, &C, 4, NULL, 0, DEV(4), DEV(6), 0, DEV(7), DEV(8), DEV(9), 0, DEV(12), NULL), GPD_EINVAL,
                  "gpd_rollout_tape_pid", "NULL", n0), "NULL actions");
    CHECK(refused(gpd_rollout_tape_pid(&P, &S, &C, 4, DEV(3), 0, DEV(4), DEV(6), 0, DEV(7), DEV(8), DEV(9), 0, ODD(DEV(12), 4), NULL), GPD_EINVAL,
                  "gpd_rollout_tape_pid", "16-byte", n0), "a tape at a 4-byte offset");
    CHECK(refused(gpd_rollout_tape_pid(&P, &S, &C, 4, DEV(3), -1, DEV(4), DEV(6), 0, DEV(7), DEV(8), DEV(9), 0, DEV(12), NULL), GPD_EINVAL,
                  "gpd_rollout_tape_pid", "strides", n0), "a negative stride");
    CHECK(refused(gpd_rollout_tape_pid(&P, &S, &C, 4, DEV(3), 0, NULL, DEV(6), 0, DEV(7), DEV(8), DEV(9), 0, DEV(12), NULL), GPD_EINVAL,
                  "gpd_rollout_tape_pid", "target_pos", n0), "the hover task without a target");
    S.kin = ODD(DEV(1), 4);
    CHECK(refused(tape_call(4), GPD_EINVAL, "gpd_rollout_tape_pid", "16-byte", n0), "state.kin at a 4-byte offset");
    S.kin = DEV(1);
    S.ld = 100;
    CHECK(refused(tape_call(4), GPD_EINVAL, "gpd_rollout_tape_pid", "ld", n0), "state.ld below the number of drones");
    S.ld = 4096;
#define VJP(ld_, K_, act_, stride_, tgt_, tape_, gk_, gp_, ga_, gg_) \
    gpd_rollout_vjp_pid(&P, &C, ld_, K_, act_, stride_, tgt_, tape_, NULL, 0, NULL, 0, gk_, gp_, ga_, gg_, NULL)
    CHECK(refused(gpd_rollout_vjp_pid(NULL, &C, S.ld, 4, DEV(3), 0, DEV(4), DEV(12), NULL, 0, NULL, 0, DEV(15), DEV(18), DEV(16), NULL, NULL), GPD_EINVAL,
                  "gpd_rollout_vjp_pid", "NULL", n0), "NULL params");
    CHECK(refused(VJP(S.ld, 4, DEV(3), 0, DEV(4), NULL, DEV(15), DEV(18), DEV(16), NULL), GPD_EINVAL, "gpd_rollout_vjp_pid", "NULL", n0), "NULL tape");
    CHECK(refused(VJP(S.ld, 4, DEV(3), 0, DEV(4), DEV(12), NULL, DEV(18), DEV(16), NULL), GPD_EINVAL, "gpd_rollout_vjp_pid", "NULL", n0), "NULL g_kin");
    CHECK(refused(VJP(S.ld, 4, DEV(3), 0, DEV(4), DEV(12), DEV(15), NULL, DEV(16), NULL), GPD_EINVAL, "gpd_rollout_vjp_pid", "NULL", n0), "NULL g_pid");
    CHECK(refused(VJP(S.ld, 4, DEV(3), 0, DEV(4), DEV(12), DEV(15), DEV(18), NULL, NULL), GPD_EINVAL, "gpd_rollout_vjp_pid", "NULL", n0), "NULL g_actions");
    CHECK(refused(VJP(S.ld, 4, DEV(3), 0, DEV(4), ODD(DEV(12), 8), DEV(15), DEV(18), DEV(16), NULL), GPD_EINVAL, "gpd_rollout_vjp_pid", "16-byte", n0),
          "a tape at an 8-byte offset");
    CHECK(refused(VJP(S.ld, 4, DEV(3), 0, DEV(4), DEV(12), ODD(DEV(15), 8), DEV(18), DEV(16), NULL), GPD_EINVAL, "gpd_rollout_vjp_pid", "16-byte", n0),
          "g_kin at an 8-byte offset");
    CHECK(refused(VJP(S.ld, 4, DEV(3), 0, DEV(4), DEV(12), DEV(15), ODD(DEV(18), 4), DEV(16), NULL), GPD_EINVAL, "gpd_rollout_vjp_pid", "16-byte", n0),
          "g_pid at a 4-byte offset");
    CHECK(refused(VJP(S.ld, 4, DEV(3), 0, DEV(4), DEV(12), DEV(15), DEV(18), DEV(16), ODD(DEV(19), 4)), GPD_EINVAL, "gpd_rollout_vjp_pid", "16-byte", n0),
          "g_gains at a 4-byte offset");
    CHECK(refused(VJP(S.ld, 4, DEV(3), 0, DEV(4), DEV(12), DEV(15), DEV(18), ODD(DEV(16), 4), NULL), GPD_EINVAL, "gpd_rollout_vjp_pid", "16-byte", n0),
          "g_actions at a 4-byte offset (VEL: its rows are stored as float4)");
    C.act_type = GPD_ACT_PID;
    CHECK(VJP(S.ld, 4, DEV(3), 0, DEV(4), DEV(12), DEV(15), DEV(18), ODD(DEV(16), 4), NULL) == 0 && hipstub_launches() == n0 + 1,
          "... which PID's scalar stores do not need");
    n0 = hipstub_launches();
    C.act_type = GPD_ACT_VEL;
    CHECK(refused(VJP(S.ld, 4, DEV(3), -1, DEV(4), DEV(12), DEV(15), DEV(18), DEV(16), NULL), GPD_EINVAL, "gpd_rollout_vjp_pid", "strides", n0),
          "a negative stride");
    CHECK(refused(VJP(S.ld, 4, DEV(3), 0, NULL, DEV(12), DEV(15), DEV(18), DEV(16), NULL), GPD_EINVAL, "gpd_rollout_vjp_pid", "target_pos", n0),
          "the hover task without a target");
    CHECK(refused(VJP(100, 4, DEV(3), 0, DEV(4), DEV(12), DEV(15), DEV(18), DEV(16), NULL), GPD_EINVAL, "gpd_rollout_vjp_pid", "ld", n0),
          "ld below the number of drones");
    CHECK(refused(VJP(0, 4, DEV(3), 0, DEV(4), DEV(12), DEV(15), DEV(18), DEV(16), NULL), GPD_EINVAL, "gpd_rollout_vjp_pid", "ld", n0), "ld = 0");
    C.act_type = 7;
    all_refuse(3, 4, GPD_EINVAL, "unknown act_type", "an action type that does not exist", n0);
    C.act_type = GPD_ACT_VEL;
    C.substeps = 0;
    all_refuse(3, 4, GPD_EINVAL, "must be positive", "no sub-steps", n0);
    C.substeps = 5;
    CHECK(hipstub_launches() == n0, "no refusal launched anything");

    C.num_envs = 1 << 26; S.ld = 1ll << 26;
    CHECK(tape_call(1) == 0 && vjp_call(1) == 0, "2^26 drones in one launch");
    hipstub_last(last);
    CHECK(last[0] == (1u << 18), "2^26 drones: 2^18 workgroups");

    if (argc > 1) CHECK(write_formulas(argv[1]) == 0, "dslpid_vjp.inc on 400 controller calls, written out; the gains flag leaves the other cotangents' bits alone");

    printf("%d checks failed\n", failed);
    return failed;
}
