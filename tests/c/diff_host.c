/*
 * Drives the HOST side of the differentiable rollout's entries (include/gpd.h: gpd_rollout_tape_floats, gpd_rollout_tape,
 * gpd_rollout_vjp) under AddressSanitizer + UndefinedBehaviorSanitizer on a machine without a GPU, the way tests/c/asan_host.c drives
 * the rest of the C-ABI: libgpd's five units compiled host-only with the sanitizers, the HIP runtime replaced by tests/stubs/hip_stub.c
 * (launches are counted and named, nothing runs).  Accepted arguments: the tape's size, one launch each, its geometry, and WHICH kernel
 * (gpd_rollout_tape_kernel / gpd_rollout_vjp_kernel <EXT, AW, PLANT>).  Rejected arguments: the code, a message that names the entry
 * and the reason, and no launch.  Device pointers are fake non-null addresses: host code must never dereference them.
 * Run by tests/test_host_diff.py.  Prints one line per check; exit code = failed checks.
 */
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include "gpd.h"

int hipstub_launches(void);
void hipstub_last(unsigned out[7]);
const char* hipstub_last_kernel(void);
#define KERNEL(piece) (strstr(hipstub_last_kernel(), piece) != NULL)

static int failed;
#define CHECK(cond, what) do { if (!(cond)) { ++failed; printf("FAIL %s (line %d): %s\n", what, __LINE__, gpd_last_error()); } else printf("ok   %s\n", what); } while (0)
#define DEV(n) ((void*)(uintptr_t)(0x100000000ull + 0x1000000ull * (n)))      /* fake device addresses */

static GpdParams P;
static GpdState S;
static GpdStepCfg C;

static int tape_call(int K) {
    return gpd_rollout_tape(&P, &S, &C, K, DEV(3), 4096 * 4, DEV(4), DEV(6), 4096 * 12, DEV(7), DEV(8), DEV(9), 4096, NULL, DEV(12), NULL);
}
static int vjp_call(int K) {
    return gpd_rollout_vjp(&P, &C, S.ld, K, DEV(3), 4096 * 4, DEV(4), NULL, DEV(12), DEV(13), 4096 * 12, DEV(14), 4096, DEV(15), DEV(16), NULL);
}
/* a rejected call: the code, the entry's name and the reason in the message, nothing launched */
static int refused(int rc, int code, const char* entry, const char* reason, int launches_before) {
    return rc == code && strncmp(gpd_last_error(), entry, strlen(entry)) == 0 && strstr(gpd_last_error(), reason) != NULL &&
           hipstub_launches() == launches_before;
}

int main(void) {
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

    /* ---- rejected configurations: GPD_ENOTSUP, the entry and the reason, nothing launched ---- */
    n0 = hipstub_launches();
    const int pid_acts[3] = {GPD_ACT_PID, GPD_ACT_VEL, GPD_ACT_ONE_D_PID};
    for (int i = 0; i < 3; ++i) {
        C.act_type = pid_acts[i];
        CHECK(refused(tape_call(4), GPD_ENOTSUP, "gpd_rollout_tape", "DSLPID", n0), "gpd_rollout_tape: a DSLPID action type");
        CHECK(refused(vjp_call(4), GPD_ENOTSUP, "gpd_rollout_vjp", "DSLPID", n0), "gpd_rollout_vjp: a DSLPID action type");
        CHECK(refused(gpd_rollout_tape_floats(&C, 4, 4096, &floats), GPD_ENOTSUP, "gpd_rollout_tape_floats", "DSLPID", n0), "gpd_rollout_tape_floats: a DSLPID action type");
    }
    C.act_type = GPD_ACT_RPM;
    const uint32_t other_flags[5] = {GPD_PHYS_GND, GPD_PHYS_DW, GPD_PHYS_GROUND, GPD_PHYS_DAMP, GPD_PHYS_DRAG | GPD_PHYS_GND};
    for (int i = 0; i < 5; ++i) {
        C.physics_flags = other_flags[i];
        CHECK(refused(tape_call(4), GPD_ENOTSUP, "gpd_rollout_tape", "physics_flags", n0), "gpd_rollout_tape: a flag besides drag");
        CHECK(refused(vjp_call(4), GPD_ENOTSUP, "gpd_rollout_vjp", "physics_flags", n0), "gpd_rollout_vjp: a flag besides drag");
    }
    C.physics_flags = 0;
    C.drones_per_env = 2; C.num_envs = 2048;
    CHECK(refused(tape_call(4), GPD_ENOTSUP, "gpd_rollout_tape", "drones_per_env", n0), "gpd_rollout_tape: aviaries of two drones");
    CHECK(refused(vjp_call(4), GPD_ENOTSUP, "gpd_rollout_vjp", "drones_per_env", n0), "gpd_rollout_vjp: aviaries of two drones");
    C.drones_per_env = 1; C.num_envs = 4096;
    C.task = GPD_TASK_MULTIHOVER;
    CHECK(refused(tape_call(4), GPD_ENOTSUP, "gpd_rollout_tape", "task", n0), "gpd_rollout_tape: the multi-drone task");
    CHECK(refused(vjp_call(4), GPD_ENOTSUP, "gpd_rollout_vjp", "task", n0), "gpd_rollout_vjp: the multi-drone task");
    C.task = GPD_TASK_HOVER;
    C.auto_reset = 1;
    CHECK(refused(tape_call(4), GPD_ENOTSUP, "gpd_rollout_tape", "auto_reset", n0), "gpd_rollout_tape: auto_reset");
    CHECK(refused(vjp_call(4), GPD_ENOTSUP, "gpd_rollout_vjp", "auto_reset", n0), "gpd_rollout_vjp: auto_reset");
    C.auto_reset = 0;
    S.dw_force = DEV(17);
    CHECK(refused(tape_call(4), GPD_ENOTSUP, "gpd_rollout_tape", "dw_force", n0), "gpd_rollout_tape: downwash computed outside the kernel");
    S.dw_force = NULL;

    /* ---- bad arguments: GPD_EINVAL / GPD_ERANGE, nothing launched ---- */
    CHECK(refused(tape_call(0), GPD_EINVAL, "gpd_rollout_tape", "num_steps", n0), "K = 0");
    CHECK(refused(vjp_call(-1), GPD_EINVAL, "gpd_rollout_vjp", "num_steps", n0), "K = -1");
    CHECK(refused(gpd_rollout_tape(&P, &S, &C, 4, DEV(3), 0, DEV(4), DEV(6), 0, DEV(7), DEV(8), DEV(9), 0, NULL, NULL, NULL), GPD_EINVAL, "gpd_rollout_tape", "NULL", n0), "NULL tape");
    CHECK(refused(gpd_rollout_tape(&P, &S, &C, 4, DEV(3), 0, DEV(4), DEV(6), 0, DEV(7), DEV(8), DEV(9), 0, NULL, (float*)((char*)DEV(12) + 4), NULL), GPD_EINVAL,
                  "gpd_rollout_tape", "16-byte", n0), "a tape at a 4-byte offset");
    CHECK(refused(gpd_rollout_tape(&P, &S, &C, 4, DEV(3), -1, DEV(4), DEV(6), 0, DEV(7), DEV(8), DEV(9), 0, NULL, DEV(12), NULL), GPD_EINVAL, "gpd_rollout_tape", "strides", n0),
          "a negative stride");
    CHECK(refused(gpd_rollout_tape(&P, &S, &C, 4, DEV(3), 0, NULL, DEV(6), 0, DEV(7), DEV(8), DEV(9), 0, NULL, DEV(12), NULL), GPD_EINVAL, "gpd_rollout_tape", "target_pos", n0),
          "the hover task without a target");
    C.physics_flags = GPD_PHYS_DRAG; S.last_rpm = NULL;
    CHECK(refused(tape_call(4), GPD_EINVAL, "gpd_rollout_tape", "last_rpm", n0), "drag without state.last_rpm");
    C.physics_flags = 0; S.last_rpm = DEV(10);
    CHECK(refused(gpd_rollout_vjp(&P, &C, S.ld, 4, DEV(3), 0, DEV(4), NULL, DEV(12), NULL, 0, NULL, 0, NULL, DEV(16), NULL), GPD_EINVAL, "gpd_rollout_vjp", "NULL", n0), "NULL g_kin");
    CHECK(refused(gpd_rollout_vjp(&P, &C, S.ld, 4, DEV(3), 0, DEV(4), NULL, DEV(12), NULL, 0, NULL, 0, (float*)((char*)DEV(15) + 8), DEV(16), NULL), GPD_EINVAL,
                  "gpd_rollout_vjp", "16-byte", n0), "g_kin at an 8-byte offset");
    CHECK(refused(gpd_rollout_vjp(&P, &C, 100, 4, DEV(3), 0, DEV(4), NULL, DEV(12), NULL, 0, NULL, 0, DEV(15), DEV(16), NULL), GPD_EINVAL, "gpd_rollout_vjp", "ld", n0), "ld below the number of drones");
    C.num_envs = (1 << 26) + 1; S.ld = (1ll << 26) + 64;
    CHECK(refused(tape_call(1), GPD_ERANGE, "gpd_rollout_tape", "2^26", n0) && refused(vjp_call(1), GPD_ERANGE, "gpd_rollout_vjp", "2^26", n0), "more than 2^26 drones");
    C.num_envs = 1 << 26; S.ld = 1ll << 26;
    CHECK(tape_call(1) == 0 && vjp_call(1) == 0, "2^26 drones in one launch");
    hipstub_last(last);
    CHECK(last[0] == (1u << 18), "2^26 drones: 2^18 workgroups");

    printf("%d checks failed\n", failed);
    return failed;
}
