/*
 * Drives the HOST side of gpd_task_eval / gpd_sizeof_ctbr_task / gpd_rollout_ctbr_task (include/gpd.h) under AddressSanitizer +
 * UndefinedBehaviorSanitizer on a machine without a GPU, the way tests/c/obst_task_host.c drives gpd_rollout_obst: libgpd's units
 * compiled host-only with the sanitizers, the HIP runtime replaced by tests/stubs/hip_stub.c (launches are counted and named, nothing
 * runs).  Accepted arguments: one launch, its geometry, and WHICH kernel (ctbr_task_kernel<EXT, PLANT>).  Rejected arguments: the code,
 * a message that names the entry and the reason, and no launch.  Device pointers are fake non-null addresses: host code must never
 * dereference them.  One line per check; exit code = failed checks.
 */
#include "host_check.h"

static GpdParams P;
static GpdCtbr B;
static GpdState S;
static GpdStepCfg C;
static GpdCtbrTask T, *task;
static const float *actions, *target, *init_pose, *plant;
static float *obs, *tobs, *reward, *cmd_out;
static uint8_t *terminated, *truncated;
static int32_t K;
static int64_t a_stride, o_stride, e_stride;
/* gpd_task_eval's own */
static const float* rows;
static const int32_t* counter;

static void defaults(void) {
    memset(&P, 0, sizeof P);
    memset(&B, 0, sizeof B);
    memset(&S, 0, sizeof S);
    memset(&C, 0, sizeof C);
    memset(&T, 0, sizeof T);
    S.kin = DEV(1); S.step_counter = DEV(2); S.last_rpm = DEV(3); S.ld = 128;
    C.num_envs = 70; C.drones_per_env = 1; C.act_type = GPD_ACT_RAW_RPM; C.substeps = 5; C.pyb_dt = 1.0f / 240; C.ctrl_dt = 1.0f / 48;
    C.inv_ctrl_dt = 48.0f; C.lanes_per_wave = 64; C.task = GPD_TASK_HOVER; C.auto_reset = 1; C.init_per_env = 1; C.target_per_env = 1;
    C.physics_flags = GPD_PHYS_GND | GPD_PHYS_DRAG | GPD_PHYS_GROUND | GPD_PHYS_DAMP;
    T.normalized = 1; T.act_scale[0] = 9.8f; T.act_bias[0] = 9.8f; T.act_scale[1] = T.act_scale[2] = T.act_scale[3] = 6.2831855f;
    task = &T;
    actions = DEV(4); target = DEV(5); init_pose = DEV(6); plant = DEV(7); obs = DEV(8); tobs = DEV(9); reward = DEV(10);
    terminated = DEV(11); truncated = DEV(12); cmd_out = DEV(13);
    K = 6; a_stride = 70 * 4; o_stride = 70 * 12; e_stride = 70;
    rows = DEV(14); counter = DEV(15);
}
static int call(void) {
    return gpd_rollout_ctbr_task(&P, &B, &S, &C, task, K, actions, a_stride, target, init_pose, plant, obs, tobs, o_stride, reward, terminated,
                                 truncated, e_stride, cmd_out, NULL);
}
static int eval(void) { return gpd_task_eval(&C, rows, counter, target, reward, terminated, truncated, NULL); }
#define REFUSED(code, reason, what) do { const int n0_ = hipstub_launches(); CHECK(refused(call(), code, "gpd_rollout_ctbr_task", reason, n0_), what); defaults(); } while (0)
#define LAUNCHES(piece, grid, what) do { const int n0_ = hipstub_launches(); unsigned g_[7]; const int rc_ = call(); hipstub_last(g_); \
    CHECK(rc_ == 0 && hipstub_launches() == n0_ + 1 && KERNEL("ctbr_task_kernel") && KERNEL(piece) && g_[0] == (grid) && g_[1] == 1 && g_[3] == 256 && \
          g_[6] == 0, what); printf("%s\n", piece); defaults(); } while (0)
#define NULL_ARG(expr, entry, what) do { const int n0_ = hipstub_launches(); CHECK(refused(expr, GPD_EINVAL, entry, "NULL", n0_), what); } while (0)
#define EVAL_REFUSED(code, reason, what) do { const int n0_ = hipstub_launches(); CHECK(refused(eval(), code, "gpd_task_eval", reason, n0_), what); defaults(); } while (0)
#define EVAL_LAUNCHES(grid, what) do { const int n0_ = hipstub_launches(); unsigned g_[7]; const int rc_ = eval(); hipstub_last(g_); \
    CHECK(rc_ == 0 && hipstub_launches() == n0_ + 1 && KERNEL("gpd_task_eval_kernel") && g_[0] == (grid) && g_[3] == 256 && g_[6] == 0, what); defaults(); } while (0)

int main(void) {
    defaults();
    int32_t size = 0;
    CHECK(gpd_sizeof_ctbr_task(&size) == 0 && size == (int32_t)sizeof(GpdCtbrTask) && size == 48 && size % 16 == 0, "gpd_sizeof_ctbr_task: 48 bytes");
    { const int n0 = hipstub_launches(); CHECK(refused(gpd_sizeof_ctbr_task(NULL), GPD_EINVAL, "gpd_sizeof_ctbr_task", "NULL", n0), "gpd_sizeof_ctbr_task(NULL)"); }

    /* ==== gpd_task_eval ==== */
    EVAL_LAUNCHES(1u, "70 aviaries, targets per aviary: one workgroup");
    C.num_envs = 257; C.target_per_env = 0;
    EVAL_LAUNCHES(2u, "257 aviaries, one target: two workgroups");
    C.task = GPD_TASK_NONE; target = NULL;
    EVAL_LAUNCHES(1u, "GPD_TASK_NONE without target_pos");
    C.substeps = 0; C.act_type = 99; C.physics_flags = 1u << 9; S.ld = 0;
    EVAL_LAUNCHES(1u, "fields the entry does not read are not checked");
    NULL_ARG(gpd_task_eval(NULL, rows, counter, target, reward, terminated, truncated, NULL), "gpd_task_eval", "task_eval: NULL cfg");
    rows = NULL; EVAL_REFUSED(GPD_EINVAL, "NULL", "task_eval: NULL obs12");
    counter = NULL; EVAL_REFUSED(GPD_EINVAL, "NULL", "task_eval: NULL counter");
    reward = NULL; EVAL_REFUSED(GPD_EINVAL, "NULL", "task_eval: NULL reward");
    terminated = NULL; EVAL_REFUSED(GPD_EINVAL, "NULL", "task_eval: NULL terminated");
    truncated = NULL; EVAL_REFUSED(GPD_EINVAL, "NULL", "task_eval: NULL truncated");
    target = NULL; EVAL_REFUSED(GPD_EINVAL, "target_pos", "task_eval: a task without target_pos");
    C.num_envs = 0; EVAL_REFUSED(GPD_EINVAL, "positive", "task_eval: num_envs 0");
    C.num_envs = -3; EVAL_REFUSED(GPD_EINVAL, "positive", "task_eval: num_envs negative");
    C.task = 7; EVAL_REFUSED(GPD_EINVAL, "unknown task", "task_eval: unknown task");
    C.task = -1; EVAL_REFUSED(GPD_EINVAL, "unknown task", "task_eval: negative task");
    rows = ODD(DEV(14), 4); EVAL_REFUSED(GPD_EINVAL, "16-byte", "task_eval: misaligned obs12");
    rows = ODD(DEV(14), 8); EVAL_REFUSED(GPD_EINVAL, "16-byte", "task_eval: obs12 aligned to 8 bytes only");
    C.drones_per_env = 2; EVAL_REFUSED(GPD_ENOTSUP, "one drone", "task_eval: aviaries of two");
    C.drones_per_env = 0; EVAL_REFUSED(GPD_ENOTSUP, "one drone", "task_eval: drones_per_env 0");
    C.task = GPD_TASK_MULTIHOVER; EVAL_REFUSED(GPD_ENOTSUP, "task", "task_eval: GPD_TASK_MULTIHOVER");
    C.num_envs = (1 << 26) + 1; EVAL_REFUSED(GPD_ERANGE, "2^26", "task_eval: more than 2^26 drones");
    C.num_envs = 1 << 26; EVAL_LAUNCHES((1u << 26) / 256u, "task_eval: exactly 2^26 drones");

    /* ==== gpd_rollout_ctbr_task, accepted: one launch of <EXT, PLANT> ==== */
    LAUNCHES("ILb1ELb1EE", 1u, "every allowed flag, a plant table, everything optional given -> <EXT, PLANT>");
    plant = NULL; C.physics_flags = GPD_PHYS_DAMP; C.num_envs = 257; S.ld = 320; a_stride = 257 * 4; o_stride = 257 * 12; e_stride = 257;
    LAUNCHES("ILb1ELb0EE", 2u, "damping alone, no plant table, 257 drones -> <EXT, no PLANT>, two workgroups");
    C.physics_flags = 0; S.last_rpm = NULL; S.bad = DEV(20);
    LAUNCHES("ILb0ELb1EE", 1u, "no flag, a plant table, no last_rpm, the guard -> <no EXT, PLANT>");
    C.physics_flags = 0; plant = NULL; task = NULL; tobs = NULL; cmd_out = NULL; C.task = GPD_TASK_NONE; target = NULL; C.auto_reset = 0; init_pose = NULL;
    C.act_type = GPD_ACT_DIRECT_RPM; a_stride = 0; o_stride = 0; e_stride = 0; K = 1; C.substeps = 1;
    LAUNCHES("ILb0ELb0EE", 1u, "nothing optional: no task struct, no task, no reset, held action, last rows only -> <no EXT, no PLANT>");
    T.normalized = 0; T.act_scale[0] = __builtin_nanf(""); a_stride = 70 * 4 + 4; o_stride = 70 * 12 + 4; e_stride = 71;
    LAUNCHES("ILb1ELb1EE", 1u, "not normalized (scale and bias are not read), strides above the minimum");

    /* ---- GPD_ENOTSUP: what narrows the entry, before any device call ---- */
    C.drones_per_env = 2; C.num_envs = 35; REFUSED(GPD_ENOTSUP, "one drone", "aviaries of two");
    C.task = GPD_TASK_MULTIHOVER; REFUSED(GPD_ENOTSUP, "task", "GPD_TASK_MULTIHOVER");
    for (int act = GPD_ACT_RPM; act <= GPD_ACT_DIRECT_RPM; ++act) {
        if (act == GPD_ACT_RAW_RPM || act == GPD_ACT_DIRECT_RPM) continue;
        C.act_type = act; REFUSED(GPD_ENOTSUP, "act_type", "another action type");
    }
    C.physics_flags = GPD_PHYS_DW; REFUSED(GPD_ENOTSUP, "downwash", "GPD_PHYS_DW alone");
    C.physics_flags |= GPD_PHYS_DW; REFUSED(GPD_ENOTSUP, "downwash", "GPD_PHYS_DW among the other flags");
    S.dw_force = DEV(21); REFUSED(GPD_ENOTSUP, "downwash", "state.dw_force");
    S.act_ring = DEV(22); REFUSED(GPD_ENOTSUP, "state.act_ring", "the action history");

    /* ---- GPD_EINVAL ---- */
    NULL_ARG(gpd_rollout_ctbr_task(NULL, &B, &S, &C, task, K, actions, 0, target, init_pose, plant, obs, tobs, 0, reward, terminated, truncated, 0, NULL, NULL), "gpd_rollout_ctbr_task", "NULL params");
    NULL_ARG(gpd_rollout_ctbr_task(&P, NULL, &S, &C, task, K, actions, 0, target, init_pose, plant, obs, tobs, 0, reward, terminated, truncated, 0, NULL, NULL), "gpd_rollout_ctbr_task", "NULL ctbr");
    NULL_ARG(gpd_rollout_ctbr_task(&P, &B, NULL, &C, task, K, actions, 0, target, init_pose, plant, obs, tobs, 0, reward, terminated, truncated, 0, NULL, NULL), "gpd_rollout_ctbr_task", "NULL state");
    NULL_ARG(gpd_rollout_ctbr_task(&P, &B, &S, NULL, task, K, actions, 0, target, init_pose, plant, obs, tobs, 0, reward, terminated, truncated, 0, NULL, NULL), "gpd_rollout_ctbr_task", "NULL cfg");
    actions = NULL; REFUSED(GPD_EINVAL, "NULL", "NULL actions");
    obs = NULL; REFUSED(GPD_EINVAL, "NULL", "NULL obs12");
    reward = NULL; REFUSED(GPD_EINVAL, "NULL", "NULL reward");
    terminated = NULL; REFUSED(GPD_EINVAL, "NULL", "NULL terminated");
    truncated = NULL; REFUSED(GPD_EINVAL, "NULL", "NULL truncated");
    S.kin = NULL; REFUSED(GPD_EINVAL, "NULL state.kin", "NULL state.kin");
    S.step_counter = NULL; REFUSED(GPD_EINVAL, "NULL state.kin", "NULL state.step_counter");
    S.kin = ODD(DEV(1), 4); REFUSED(GPD_EINVAL, "16-byte", "misaligned state.kin");
    S.ld = 69; REFUSED(GPD_EINVAL, "state.ld", "state.ld < num_envs");
    S.ld = 0; REFUSED(GPD_EINVAL, "state.ld", "state.ld 0");
    S.last_rpm = NULL; REFUSED(GPD_EINVAL, "GPD_PHYS_DRAG needs state.last_rpm", "drag without last_rpm");
    target = NULL; REFUSED(GPD_EINVAL, "target_pos", "a task without target_pos");
    init_pose = NULL; REFUSED(GPD_EINVAL, "init_pose", "auto_reset without init_pose");
    K = 0; REFUSED(GPD_EINVAL, "num_steps", "num_steps 0");
    K = -2; REFUSED(GPD_EINVAL, "num_steps", "num_steps negative");
    a_stride = -4; REFUSED(GPD_EINVAL, "non-negative", "a negative action stride");
    o_stride = -12; REFUSED(GPD_EINVAL, "non-negative", "a negative obs stride");
    e_stride = -1; REFUSED(GPD_EINVAL, "non-negative", "a negative env stride");
    C.num_envs = 0; REFUSED(GPD_EINVAL, "positive", "num_envs 0");
    C.substeps = 0; REFUSED(GPD_EINVAL, "positive", "substeps 0");
    C.task = 7; REFUSED(GPD_EINVAL, "unknown task", "unknown task");
    C.physics_flags = 32; REFUSED(GPD_EINVAL, "unknown physics flag", "an unknown physics flag");
    a_stride = 69 * 4; REFUSED(GPD_EINVAL, "stride", "an action stride below 4*num_envs");
    o_stride = 69 * 12; REFUSED(GPD_EINVAL, "stride", "an obs stride below 12*num_envs");
    e_stride = 69; REFUSED(GPD_EINVAL, "stride", "an env stride below num_envs");
    a_stride = 70 * 4 + 2; REFUSED(GPD_EINVAL, "multiples of 4", "an action stride that is no multiple of 4");
    o_stride = 70 * 12 + 1; REFUSED(GPD_EINVAL, "multiples of 4", "an obs stride that is no multiple of 4");
    actions = ODD(DEV(4), 4); REFUSED(GPD_EINVAL, "aligned", "misaligned actions");
    obs = ODD(DEV(8), 8); REFUSED(GPD_EINVAL, "aligned", "misaligned obs12");
    tobs = ODD(DEV(9), 4); REFUSED(GPD_EINVAL, "aligned", "misaligned term_obs12");
    plant = ODD(DEV(7), 12); REFUSED(GPD_EINVAL, "aligned", "misaligned plant_rows");
    cmd_out = ODD(DEV(13), 4); REFUSED(GPD_EINVAL, "aligned", "misaligned cmd_out");
    cmd_out = (float*)DEV(4); REFUSED(GPD_EINVAL, "alias", "cmd_out == actions");
    tobs = (float*)DEV(8); REFUSED(GPD_EINVAL, "alias", "term_obs12 == obs12");
    C.ctrl_dt = 0.0f; REFUSED(GPD_EINVAL, "positive", "ctrl_dt 0");
    C.pyb_dt = -1.0f; REFUSED(GPD_EINVAL, "positive", "pyb_dt negative");
    T.normalized = 2; REFUSED(GPD_EINVAL, "normalized", "normalized 2");
    T.normalized = -1; REFUSED(GPD_EINVAL, "normalized", "normalized -1");

    /* ---- GPD_ERANGE ---- */
    C.num_envs = (1 << 26) + 1; S.ld = (1 << 26) + 64; a_stride = o_stride = e_stride = 0; REFUSED(GPD_ERANGE, "2^26", "more than 2^26 drones");

    /* ---- gpd_rollout_ctbr still refuses a task and the auto-reset: nothing existing changed ---- */
    {
        int n0 = hipstub_launches();
        CHECK(refused(gpd_rollout_ctbr(&P, &B, &S, &C, GPD_CTBR_CMD, actions, 0, NULL, obs, 0, NULL, K, NULL), GPD_ENOTSUP, "gpd_rollout_ctbr", "GPD_TASK_NONE", n0),
              "gpd_rollout_ctbr with a task");
    }
    printf("%d checks failed\n", failed);
    return failed;
}
