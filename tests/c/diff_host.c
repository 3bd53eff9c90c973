/*
 * Drives the HOST side of the differentiable rollout's five entries (include/gpd.h: gpd_rollout_tape_floats, gpd_rollout_tape,
 * gpd_rollout_vjp, gpd_rollout_vjp_plant, gpd_plant_derive_vjp) under AddressSanitizer + UndefinedBehaviorSanitizer on a machine without
 * a GPU, the way tests/c/asan_host.c drives the rest of the C-ABI: libgpd's five units compiled host-only with the sanitizers, the HIP
 * runtime replaced by tests/stubs/hip_stub.c (launches are counted and named, nothing runs).  Accepted arguments: the tape's size, one
 * launch each, its geometry, and WHICH kernel (gpd_rollout_tape_kernel<EXT, AW, PLANT>, gpd_rollout_vjp_kernel<EXT, AW, PLANT, GP>:
 * gpd_rollout_vjp launches <.., GP 0>, gpd_rollout_vjp_plant the four <.., PLANT 1, GP 1>; gpd_plant_derive_vjp_kernel).  Rejected
 * arguments: the code, a message that names the entry and the reason, and no launch; what diff_cfg refuses for every entry is one table
 * of entries.  Device pointers are fake non-null addresses: host code must never dereference them.
 * With a file name as its argument it also evaluates csrc/plant_derive_vjp.inc -- the text the device kernel compiles -- on drones it
 * draws itself and writes inputs and outputs there, one drone per line, for tests/test_host_sysid.py to hold against a numerical
 * float64 Jacobian of the derive formulas.
 * Run once for tests/test_host_diff.py and tests/test_host_sysid.py (tests/helpers/host_lib.py).  Prints one line per check; exit code =
 * failed checks.
 */
#include "host_check.h"
#include "plant_derive_vjp.inc"

static GpdParams P;
static GpdState S;
static GpdStepCfg C;

static int tape_call(int K) {
    return gpd_rollout_tape(&P, &S, &C, K, DEV(3), 4096 * 4, DEV(4), DEV(6), 4096 * 12, DEV(7), DEV(8), DEV(9), 4096, NULL, DEV(12), NULL);
}
static int vjp_call(int K) {
    return gpd_rollout_vjp(&P, &C, S.ld, K, DEV(3), 4096 * 4, DEV(4), NULL, DEV(12), DEV(13), 4096 * 12, DEV(14), 4096, DEV(15), DEV(16), NULL);
}
static int plant_call(int K, const float* plant, float* g_plant) {
    return gpd_rollout_vjp_plant(&P, &C, S.ld, K, DEV(3), 4096 * 4, DEV(4), plant, DEV(12), DEV(13), 4096 * 12, DEV(14), 4096, DEV(15), DEV(16),
                                 g_plant, NULL);
}
static int plant_rows_call(int K) { return plant_call(K, DEV(11), DEV(17)); }
static int floats_call(int K) { int64_t floats; return gpd_rollout_tape_floats(&C, K, 4096, &floats); }
static int derive_call(int32_t n, int64_t ld) { return gpd_plant_derive_vjp(&P, DEV(20), DEV(21), n, ld, DEV(22), NULL); }

/* the entries that share diff_cfg's refusals; `prefix`: what the check lines of an entry start with where a line names its entry */
static const struct { const char* name; int (*call)(int K); const char* prefix; } ENTRIES[4] = {
    {"gpd_rollout_tape", tape_call, "gpd_rollout_tape: "}, {"gpd_rollout_vjp", vjp_call, "gpd_rollout_vjp: "},
    {"gpd_rollout_vjp_plant", plant_rows_call, ""}, {"gpd_rollout_tape_floats", floats_call, "gpd_rollout_tape_floats: "}};
/* the first `entries` of them refuse the configuration as it stands: the code, the entry and the reason, nothing launched */
static void all_refuse(int entries, int K, int code, const char* reason, int named, const char* what, int n0) {
    char line[128];
    for (int e = 0; e < entries; ++e) {
        snprintf(line, sizeof line, "%s%s", named ? ENTRIES[e].prefix : "", what);
        CHECK(refused(ENTRIES[e].call(K), code, ENTRIES[e].name, reason, n0), line);
    }
}

/* the formulas on the host: 64 drones, scales in [0.5, 2), cotangents in [-1, 1), a made-up nominal airframe of ordinary magnitudes */
static double draw(uint64_t* x) { *x = *x * 6364136223846793005ull + 1442695040888963407ull; return (double)(*x >> 11) / 9007199254740992.0; }
static int write_formulas(const char* path) {
    GpdParams N;
    memset(&N, 0, sizeof N);
    N.M = 0.027f; N.inv_M = 1.0f / 0.027f; N.KF = 3.16e-10f; N.GRAVITY = 0.26487f; N.km_over_kf = 0.025f; N.gnd_eff_coeff = 11.36859f;
    N.J[0] = 1.4e-5f; N.J[1] = 1.5e-5f; N.J[2] = 2.17e-5f;
    N.J_INV[0] = 1.0f / 1.4e-5f; N.J_INV[1] = 1.0f / 1.5e-5f; N.J_INV[2] = 1.0f / 2.17e-5f;
    N.drag_coeff[0] = 9.1785e-7f; N.drag_coeff[1] = 9.2e-7f; N.drag_coeff[2] = 10.311e-7f;
    N.hover_thrust = 0.0662175f; N.hover_resid = -3.1e-9f;
    FILE* f = fopen(path, "w");
    if (!f) return 1;
    fprintf(f, "%.9g %.9g %.9g %.9g %.9g %.9g %.9g %.9g %.9g %.9g %.9g %.9g %.9g %.9g %.9g %.9g %.9g\n", N.M, N.inv_M, N.KF, N.GRAVITY,
            N.J[0], N.J[1], N.J[2], N.J_INV[0], N.J_INV[1], N.J_INV[2], N.km_over_kf, N.gnd_eff_coeff, N.drag_coeff[0], N.drag_coeff[1],
            N.drag_coeff[2], N.hover_thrust, N.hover_resid);
    uint64_t seed = 12345;
    for (int d = 0; d < 64; ++d) {
        double s[GPD_NUM_SCALES], g[GPD_PLANT_ROWS], out[GPD_NUM_SCALES];
        for (int k = 0; k < GPD_NUM_SCALES; ++k) s[k] = 0.5 + 1.5 * draw(&seed);
        for (int r = 0; r < GPD_PLANT_ROWS; ++r) g[r] = 2.0 * draw(&seed) - 1.0;
        gpd_plant_derive_vjp_one(&N, s, g, out);
        for (int k = 0; k < GPD_NUM_SCALES; ++k) fprintf(f, "%.17g ", s[k]);
        for (int r = 0; r < GPD_PLANT_ROWS; ++r) fprintf(f, "%.17g ", g[r]);
        for (int k = 0; k < GPD_NUM_SCALES; ++k) fprintf(f, "%.17g%c", out[k], k + 1 < GPD_NUM_SCALES ? ' ' : '\n');
    }
    return fclose(f) != 0;
}

int main(int argc, char** argv) {
    memset(&P, 0, sizeof P);
    memset(&S, 0, sizeof S);
    memset(&C, 0, sizeof C);
    unsigned last[7];
    S.kin = DEV(1); S.step_counter = DEV(2); S.ld = 4096; S.last_rpm = DEV(10);
    C.num_envs = 4096; C.drones_per_env = 1; C.substeps = 8; C.act_type = GPD_ACT_RPM; C.task = GPD_TASK_HOVER; C.pyb_dt = 1.0f / 240;
    C.ctrl_dt = 1.0f / 30; C.inv_ctrl_dt = 30;

    /* ---- the size query ---- */
    int64_t floats = -1;
    CHECK(gpd_rollout_tape_floats(&C, 20, 4096, &floats) == 0 && floats == (13 * 20 + 1) * 4096LL, "tape of 20 steps: 13 rows per step + 1, times ld");
    CHECK(gpd_rollout_tape_floats(&C, 1, 70 + 58, &floats) == GPD_EINVAL, "ld below the number of drones");
    C.num_envs = 70;
    CHECK(gpd_rollout_tape_floats(&C, 1, 128, &floats) == 0 && floats == 14 * 128, "70 drones at ld = 128, one step");
    C.num_envs = 4096;
    CHECK(gpd_rollout_tape_floats(NULL, 1, 4096, &floats) == GPD_EINVAL && gpd_rollout_tape_floats(&C, 1, 4096, NULL) == GPD_EINVAL, "NULL cfg / floats_out");
    CHECK(gpd_rollout_tape_floats(&C, 0, 4096, &floats) == GPD_EINVAL, "num_steps 0");
    CHECK(gpd_rollout_tape_floats(&C, 2147483647, 0xffffffffLL, &floats) == GPD_ERANGE, "a tape beyond 2^63 floats -> GPD_ERANGE");
    CHECK(gpd_rollout_tape_floats(&C, 1, 1ll << 32, &floats) == GPD_EINVAL, "a pitch beyond 2^32 - 1");

    /* ---- accepted calls: one launch each, the kernel named ---- */
    int n0 = hipstub_launches();
    CHECK(tape_call(20) == 0 && hipstub_launches() == n0 + 1, "gpd_rollout_tape launches once");
    hipstub_last(last);
    CHECK(last[0] == 16 && last[3] == 256 && last[6] == 0, "4096 drones: 16 workgroups of 256 lanes, no dynamic LDS");
    CHECK(KERNEL("gpd_rollout_tape_kernelILb0ELi4ELb0E"), "RPM, no flags, nominal airframe -> gpd_rollout_tape_kernel<EXT 0, AW 4, PLANT 0>");
    CHECK(vjp_call(20) == 0 && hipstub_launches() == n0 + 2, "gpd_rollout_vjp launches once");
    hipstub_last(last);
    CHECK(last[0] == 16 && last[3] == 256 && last[6] == 0, "the reverse sweep: one lane per drone");
    CHECK(KERNEL("gpd_rollout_vjp_kernelILb0ELi4ELb0E"), "-> gpd_rollout_vjp_kernel<EXT 0, AW 4, PLANT 0>");
    CHECK(gpd_rollout_vjp(&P, &C, S.ld, 20, DEV(3), 0, DEV(4), NULL, DEV(12), NULL, 0, NULL, 0, DEV(15), DEV(16), NULL) == 0,
          "NULL cotangents of obs12 and reward (zeros), a shared action block");
    C.physics_flags = GPD_PHYS_DRAG; C.act_type = GPD_ACT_ONE_D_RPM;
    CHECK(tape_call(3) == 0 && KERNEL("gpd_rollout_tape_kernelILb1ELi1ELb0E"), "ONE_D_RPM with drag -> <EXT 1, AW 1, PLANT 0>");
    CHECK(vjp_call(3) == 0 && KERNEL("gpd_rollout_vjp_kernelILb1ELi1ELb0E"), "... and its reverse sweep");
    C.physics_flags = 0;
    for (int act = GPD_ACT_RAW_RPM; act <= GPD_ACT_DIRECT_RPM; ++act) {
        C.act_type = act;
        CHECK(gpd_rollout_tape(&P, &S, &C, 1, DEV(3), 0, DEV(4), DEV(6), 0, DEV(7), DEV(8), DEV(9), 0, DEV(11), DEV(12), NULL) == 0 &&
              KERNEL("gpd_rollout_tape_kernelILb0ELi4ELb1E"), "raw RPMs with a plant table -> <EXT 0, AW 4, PLANT 1>");
        CHECK(gpd_rollout_vjp(&P, &C, S.ld, 1, DEV(3), 0, DEV(4), DEV(11), DEV(12), DEV(13), 0, DEV(14), 0, DEV(15), DEV(16), NULL) == 0 &&
              KERNEL("gpd_rollout_vjp_kernelILb0ELi4ELb1E"), "... and its reverse sweep");
    }
    C.act_type = GPD_ACT_RPM; C.task = GPD_TASK_NONE;
    CHECK(gpd_rollout_tape(&P, &S, &C, 5, DEV(3), 4096 * 4, NULL, DEV(6), 4096 * 12, DEV(7), DEV(8), DEV(9), 4096, NULL, DEV(12), NULL) == 0,
          "no task needs no target");
    CHECK(gpd_rollout_vjp(&P, &C, S.ld, 5, DEV(3), 4096 * 4, NULL, NULL, DEV(12), DEV(13), 4096 * 12, NULL, 0, DEV(15), DEV(16), NULL) == 0,
          "... in the reverse sweep either");
    C.task = GPD_TASK_HOVER;

    /* ---- ... and of the plant-gradient entries ---- */
    n0 = hipstub_launches();
    CHECK(plant_call(20, DEV(11), DEV(17)) == 0 && hipstub_launches() == n0 + 1, "gpd_rollout_vjp_plant launches once");
    hipstub_last(last);
    CHECK(last[0] == 16 && last[3] == 256 && last[6] == 0, "4096 drones: 16 workgroups of 256 lanes, no dynamic LDS");
    CHECK(KERNEL("gpd_rollout_vjp_kernelILb0ELi4ELb1ELb1E"), "RPM, no flags -> gpd_rollout_vjp_kernel<EXT 0, AW 4, PLANT 1, GP 1>");
    C.act_type = GPD_ACT_ONE_D_RPM;
    CHECK(plant_call(3, DEV(11), DEV(17)) == 0 && KERNEL("gpd_rollout_vjp_kernelILb0ELi1ELb1ELb1E"), "ONE_D_RPM -> <EXT 0, AW 1, PLANT 1, GP 1>");
    C.physics_flags = GPD_PHYS_DRAG;
    CHECK(plant_call(3, DEV(11), DEV(17)) == 0 && KERNEL("gpd_rollout_vjp_kernelILb1ELi1ELb1ELb1E"), "ONE_D_RPM with drag -> <EXT 1, AW 1, PLANT 1, GP 1>");
    for (int act = GPD_ACT_RAW_RPM; act <= GPD_ACT_DIRECT_RPM; ++act) {
        C.act_type = act;
        CHECK(plant_call(1, DEV(11), DEV(17)) == 0 && KERNEL("gpd_rollout_vjp_kernelILb1ELi4ELb1ELb1E"), "raw RPMs with drag -> <EXT 1, AW 4, PLANT 1, GP 1>");
    }
    C.act_type = GPD_ACT_RPM; C.physics_flags = 0;
    CHECK(gpd_rollout_vjp_plant(&P, &C, S.ld, 5, DEV(3), 0, DEV(4), DEV(11), DEV(12), NULL, 0, NULL, 0, DEV(15), DEV(16), DEV(17), NULL) == 0,
          "NULL cotangents of obs12 and reward (zeros), a shared action block");
    C.task = GPD_TASK_NONE;
    CHECK(gpd_rollout_vjp_plant(&P, &C, S.ld, 5, DEV(3), 4096 * 4, NULL, DEV(11), DEV(12), DEV(13), 4096 * 12, NULL, 0, DEV(15), DEV(16), DEV(17), NULL) == 0,
          "no task needs no target");
    C.task = GPD_TASK_HOVER;
    /* the sweep without the rows' cotangents is the kernel it was, with or without a plant table */
    CHECK(gpd_rollout_vjp(&P, &C, S.ld, 4, DEV(3), 0, DEV(4), DEV(11), DEV(12), NULL, 0, NULL, 0, DEV(15), DEV(16), NULL) == 0 &&
          KERNEL("gpd_rollout_vjp_kernelILb0ELi4ELb1ELb0E"), "gpd_rollout_vjp with a plant table -> <EXT 0, AW 4, PLANT 1, GP 0>");
    CHECK(gpd_rollout_vjp(&P, &C, S.ld, 4, DEV(3), 0, DEV(4), NULL, DEV(12), NULL, 0, NULL, 0, DEV(15), DEV(16), NULL) == 0 &&
          KERNEL("gpd_rollout_vjp_kernelILb0ELi4ELb0ELb0E"), "gpd_rollout_vjp without one -> <EXT 0, AW 4, PLANT 0, GP 0>");
    n0 = hipstub_launches();
    CHECK(derive_call(4096, S.ld) == 0 && hipstub_launches() == n0 + 1 && KERNEL("gpd_plant_derive_vjp_kernel"), "gpd_plant_derive_vjp launches its kernel once");
    hipstub_last(last);
    CHECK(last[0] == 16 && last[3] == 256 && last[6] == 0, "one lane per drone: 16 workgroups of 256");
    CHECK(derive_call(70, 128) == 0, "70 drones at ld = 128");
    hipstub_last(last);
    CHECK(last[0] == 1, "... one workgroup");
    CHECK(derive_call(1 << 26, 1ll << 26) == 0, "2^26 drones in one launch");
    hipstub_last(last);
    CHECK(last[0] == (1u << 18), "... 2^18 workgroups");

    /* ---- rejected configurations: GPD_ENOTSUP from every entry (the size query: where it depends on what is refused), nothing launched ---- */
    n0 = hipstub_launches();
    const int pid_acts[3] = {GPD_ACT_PID, GPD_ACT_VEL, GPD_ACT_ONE_D_PID};
    for (int i = 0; i < 3; ++i) {
        C.act_type = pid_acts[i];
        all_refuse(4, 4, GPD_ENOTSUP, "DSLPID", 1, "a DSLPID action type", n0);
    }
    C.act_type = GPD_ACT_RPM;
    const uint32_t other_flags[5] = {GPD_PHYS_GND, GPD_PHYS_DW, GPD_PHYS_GROUND, GPD_PHYS_DAMP, GPD_PHYS_DRAG | GPD_PHYS_GND};
    for (int i = 0; i < 5; ++i) {
        C.physics_flags = other_flags[i];
        all_refuse(3, 4, GPD_ENOTSUP, "physics_flags", 1, "a flag besides drag", n0);
    }
    C.physics_flags = 0;
    C.drones_per_env = 2; C.num_envs = 2048;
    all_refuse(3, 4, GPD_ENOTSUP, "drones_per_env", 1, "aviaries of two drones", n0);
    C.drones_per_env = 1; C.num_envs = 4096;
    C.task = GPD_TASK_MULTIHOVER;
    all_refuse(3, 4, GPD_ENOTSUP, "task", 1, "the multi-drone task", n0);
    C.task = GPD_TASK_HOVER;
    C.auto_reset = 1;
    all_refuse(3, 4, GPD_ENOTSUP, "auto_reset", 1, "auto_reset", n0);
    C.auto_reset = 0;
    C.num_envs = (1 << 26) + 1; S.ld = (1ll << 26) + 64;
    all_refuse(3, 1, GPD_ERANGE, "2^26", 0, "more than 2^26 drones", n0);
    C.num_envs = 4096; S.ld = 4096;
    S.dw_force = DEV(17);
    CHECK(refused(tape_call(4), GPD_ENOTSUP, "gpd_rollout_tape", "dw_force", n0), "gpd_rollout_tape: downwash computed outside the kernel");
    S.dw_force = NULL;

    /* ---- bad arguments: GPD_EINVAL / GPD_ERANGE, nothing launched ---- */
    CHECK(refused(tape_call(0), GPD_EINVAL, "gpd_rollout_tape", "num_steps", n0), "K = 0");
    CHECK(refused(vjp_call(-1), GPD_EINVAL, "gpd_rollout_vjp", "num_steps", n0), "K = -1");
    CHECK(refused(gpd_rollout_tape(&P, &S, &C, 4, DEV(3), 0, DEV(4), DEV(6), 0, DEV(7), DEV(8), DEV(9), 0, NULL, NULL, NULL), GPD_EINVAL, "gpd_rollout_tape", "NULL", n0), "NULL tape");
    CHECK(refused(gpd_rollout_tape(&P, &S, &C, 4, DEV(3), 0, DEV(4), DEV(6), 0, DEV(7), DEV(8), DEV(9), 0, NULL, ODD(DEV(12), 4), NULL), GPD_EINVAL,
                  "gpd_rollout_tape", "16-byte", n0), "a tape at a 4-byte offset");
    CHECK(refused(gpd_rollout_tape(&P, &S, &C, 4, DEV(3), -1, DEV(4), DEV(6), 0, DEV(7), DEV(8), DEV(9), 0, NULL, DEV(12), NULL), GPD_EINVAL, "gpd_rollout_tape", "strides", n0),
          "a negative stride");
    CHECK(refused(gpd_rollout_tape(&P, &S, &C, 4, DEV(3), 0, NULL, DEV(6), 0, DEV(7), DEV(8), DEV(9), 0, NULL, DEV(12), NULL), GPD_EINVAL, "gpd_rollout_tape", "target_pos", n0),
          "the hover task without a target");
    C.physics_flags = GPD_PHYS_DRAG; S.last_rpm = NULL;
    CHECK(refused(tape_call(4), GPD_EINVAL, "gpd_rollout_tape", "last_rpm", n0), "drag without state.last_rpm");
    C.physics_flags = 0; S.last_rpm = DEV(10);
    CHECK(refused(gpd_rollout_vjp(&P, &C, S.ld, 4, DEV(3), 0, DEV(4), NULL, DEV(12), NULL, 0, NULL, 0, NULL, DEV(16), NULL), GPD_EINVAL, "gpd_rollout_vjp", "NULL", n0), "NULL g_kin");
    CHECK(refused(gpd_rollout_vjp(&P, &C, S.ld, 4, DEV(3), 0, DEV(4), NULL, DEV(12), NULL, 0, NULL, 0, ODD(DEV(15), 8), DEV(16), NULL), GPD_EINVAL,
                  "gpd_rollout_vjp", "16-byte", n0), "g_kin at an 8-byte offset");
    CHECK(refused(gpd_rollout_vjp(&P, &C, 100, 4, DEV(3), 0, DEV(4), NULL, DEV(12), NULL, 0, NULL, 0, DEV(15), DEV(16), NULL), GPD_EINVAL, "gpd_rollout_vjp", "ld", n0), "ld below the number of drones");

    /* ---- gpd_rollout_vjp_plant: what it refuses, nothing launched ---- */
    CHECK(refused(plant_call(4, NULL, DEV(17)), GPD_EINVAL, "gpd_rollout_vjp_plant", "plant_rows", n0), "no plant table");
    CHECK(refused(plant_call(4, DEV(11), NULL), GPD_EINVAL, "gpd_rollout_vjp_plant", "g_plant_rows", n0), "NULL g_plant_rows");
    CHECK(refused(plant_call(4, DEV(11), ODD(DEV(17), 4)), GPD_EINVAL, "gpd_rollout_vjp_plant", "16-byte", n0), "g_plant_rows at a 4-byte offset");
    CHECK(refused(plant_call(4, ODD(DEV(11), 8), DEV(17)), GPD_EINVAL, "gpd_rollout_vjp_plant", "16-byte", n0), "plant_rows at an 8-byte offset");
    CHECK(refused(gpd_rollout_vjp_plant(NULL, &C, S.ld, 4, DEV(3), 0, DEV(4), DEV(11), DEV(12), NULL, 0, NULL, 0, DEV(15), DEV(16), DEV(17), NULL), GPD_EINVAL,
                  "gpd_rollout_vjp_plant", "NULL", n0), "NULL params");
    CHECK(refused(gpd_rollout_vjp_plant(&P, &C, S.ld, 4, DEV(3), 0, DEV(4), DEV(11), DEV(12), NULL, 0, NULL, 0, NULL, DEV(16), DEV(17), NULL), GPD_EINVAL,
                  "gpd_rollout_vjp_plant", "NULL", n0), "NULL g_kin");
    CHECK(refused(gpd_rollout_vjp_plant(&P, &C, S.ld, 4, DEV(3), 0, DEV(4), DEV(11), DEV(12), NULL, 0, NULL, 0, ODD(DEV(15), 8), DEV(16), DEV(17), NULL), GPD_EINVAL,
                  "gpd_rollout_vjp_plant", "16-byte", n0), "g_kin at an 8-byte offset");
    CHECK(refused(gpd_rollout_vjp_plant(&P, &C, S.ld, 4, DEV(3), 0, NULL, DEV(11), DEV(12), NULL, 0, NULL, 0, DEV(15), DEV(16), DEV(17), NULL), GPD_EINVAL,
                  "gpd_rollout_vjp_plant", "target_pos", n0), "the hover task without a target");
    CHECK(refused(gpd_rollout_vjp_plant(&P, &C, 100, 4, DEV(3), 0, DEV(4), DEV(11), DEV(12), NULL, 0, NULL, 0, DEV(15), DEV(16), DEV(17), NULL), GPD_EINVAL,
                  "gpd_rollout_vjp_plant", "ld", n0), "ld below the number of drones");
    CHECK(refused(gpd_rollout_vjp_plant(&P, &C, S.ld, 4, DEV(3), -1, DEV(4), DEV(11), DEV(12), NULL, 0, NULL, 0, DEV(15), DEV(16), DEV(17), NULL), GPD_EINVAL,
                  "gpd_rollout_vjp_plant", "strides", n0), "a negative stride");
    CHECK(refused(plant_call(0, DEV(11), DEV(17)), GPD_EINVAL, "gpd_rollout_vjp_plant", "num_steps", n0), "K = 0");

    /* ---- gpd_plant_derive_vjp: what it refuses ---- */
    CHECK(refused(gpd_plant_derive_vjp(NULL, DEV(20), DEV(21), 70, 128, DEV(22), NULL), GPD_EINVAL, "gpd_plant_derive_vjp", "NULL", n0), "NULL nominal");
    CHECK(refused(gpd_plant_derive_vjp(&P, NULL, DEV(21), 70, 128, DEV(22), NULL), GPD_EINVAL, "gpd_plant_derive_vjp", "NULL", n0), "NULL scales");
    CHECK(refused(gpd_plant_derive_vjp(&P, DEV(20), NULL, 70, 128, DEV(22), NULL), GPD_EINVAL, "gpd_plant_derive_vjp", "NULL", n0), "NULL g_rows");
    CHECK(refused(gpd_plant_derive_vjp(&P, DEV(20), DEV(21), 70, 128, NULL, NULL), GPD_EINVAL, "gpd_plant_derive_vjp", "NULL", n0), "NULL g_scales");
    CHECK(refused(derive_call(0, 128), GPD_EINVAL, "gpd_plant_derive_vjp", "n must", n0), "n = 0");
    CHECK(refused(derive_call(-1, 128), GPD_EINVAL, "gpd_plant_derive_vjp", "n must", n0), "n = -1");
    CHECK(refused(derive_call(70, 64), GPD_EINVAL, "gpd_plant_derive_vjp", "ld", n0), "ld below the number of drones");
    CHECK(refused(derive_call(70, 0), GPD_EINVAL, "gpd_plant_derive_vjp", "ld", n0), "ld = 0");
    CHECK(refused(derive_call(70, 1ll << 32), GPD_EINVAL, "gpd_plant_derive_vjp", "ld", n0), "a pitch beyond 2^32 - 1");
    CHECK(refused(derive_call((1 << 26) + 1, (1ll << 26) + 64), GPD_ERANGE, "gpd_plant_derive_vjp", "2^26", n0), "more than 2^26 drones");
    CHECK(hipstub_launches() == n0, "no refusal launched anything");

    C.num_envs = 1 << 26; S.ld = 1ll << 26;
    CHECK(tape_call(1) == 0 && vjp_call(1) == 0, "2^26 drones in one launch");
    hipstub_last(last);
    CHECK(last[0] == (1u << 18), "2^26 drones: 2^18 workgroups");

    if (argc > 1) CHECK(write_formulas(argv[1]) == 0, "the formulas of plant_derive_vjp.inc on 64 drones, written out");

    printf("%d checks failed\n", failed);
    return failed;
}
