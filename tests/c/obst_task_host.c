/*
 * Drives the HOST side of gpd_rollout_obst (include/gpd.h) under AddressSanitizer + UndefinedBehaviorSanitizer on a machine without a
 * GPU, the way tests/c/mppi_plant_host.c drives gpd_mppi_plant: libgpd's units compiled host-only with the sanitizers, the HIP runtime
 * replaced by tests/stubs/hip_stub.c (launches are counted and named, nothing runs).  Accepted arguments: one launch, its geometry
 * (256 / G drones per workgroup of 256, G the smallest power of two >= max(1, n_rays); a shared list's bytes of LDS), and WHICH kernel
 * (obst_task_kernel<ACT, EXT, SHARED>: ACT 0 RPM, 1 PID, 2 VEL).  Rejected arguments: the code, a message that names the entry and the
 * reason, and no launch.  Device pointers are fake non-null addresses: host code must never dereference them.
 * It also evaluates csrc/obst_task_math.inc -- the text the device kernel compiles:
 *   obst_task_host math IN OUT     IN: int32 count, then count x 6 floats task_reward, d, r, hit_reward, prox_margin, prox_weight;
 *                                  OUT: count x (float reward, float hinge, int32 hit)
 * One line per check; exit code = failed checks.
 */
#include <stdlib.h>

#include "host_check.h"
#include "obst_task_math.inc"

static GpdParams P;
static GpdState S;
static GpdStepCfg C;
static GpdObstTask Q;
static const float *actions, *target, *init_pose, *obst, *ray_dirs;
static float *rows, *reward;
static uint8_t *terminated, *truncated, *collided;
static int32_t num_steps, n_obst;
static int64_t a_stride, obst_ld, row_ld, row_stride, env_stride;

static void defaults(void) {
    memset(&P, 0, sizeof P);
    memset(&S, 0, sizeof S);
    memset(&C, 0, sizeof C);
    memset(&Q, 0, sizeof Q);
    P.pid_kf = 3.16e-10f;
    S.kin = DEV(1); S.step_counter = DEV(2); S.pid = DEV(3); S.last_rpm = DEV(4); S.ld = 128;
    C.num_envs = 70; C.drones_per_env = 1; C.act_type = GPD_ACT_VEL; C.substeps = 5; C.pyb_dt = 1.0f / 240; C.ctrl_dt = 1.0f / 48;
    C.inv_ctrl_dt = 48.0f; C.lanes_per_wave = 64; C.task = GPD_TASK_HOVER; C.auto_reset = 1; C.init_per_env = 1;
    C.physics_flags = GPD_PHYS_GND | GPD_PHYS_DRAG | GPD_PHYS_GROUND | GPD_PHYS_DAMP;
    Q.collision_radius = 0.06f; Q.hit_terminates = 1; Q.hit_reward = -5.0f; Q.prox_margin = 0.5f; Q.prox_weight = 2.0f;
    Q.n_rays = 16; Q.ray_frame = GPD_RAY_BODY; Q.max_range = 1.5f;
    actions = DEV(5); target = DEV(6); init_pose = DEV(7); obst = DEV(8); ray_dirs = DEV(9);
    rows = DEV(10); reward = DEV(11); terminated = DEV(12); truncated = DEV(13); collided = DEV(14);
    num_steps = 5; n_obst = 7; a_stride = 70 * 4; obst_ld = 1; row_ld = 32; row_stride = 70 * 32; env_stride = 70;
}
static int call(void) {
    return gpd_rollout_obst(&P, &S, &C, &Q, num_steps, actions, a_stride, target, init_pose, obst, n_obst, obst_ld, ray_dirs, rows, row_ld,
                            row_stride, reward, terminated, truncated, collided, env_stride, NULL);
}
#define REFUSED(code, reason, what) do { const int n0_ = hipstub_launches(); CHECK(refused(call(), code, "gpd_rollout_obst", reason, n0_), what); defaults(); } while (0)
#define LAUNCHES(piece, grid, lds, what) do { const int n0_ = hipstub_launches(); unsigned g_[7]; const int rc_ = call(); hipstub_last(g_); \
    CHECK(rc_ == 0 && hipstub_launches() == n0_ + 1 && KERNEL("obst_task_kernel") && KERNEL(piece) && g_[0] == (grid) && g_[1] == 1 && g_[3] == 256 && \
          g_[6] == (lds), what); printf("%s\n", piece); defaults(); } while (0)
#define NULL_ARG(expr, what) do { const int n0_ = hipstub_launches(); CHECK(refused(expr, GPD_EINVAL, "gpd_rollout_obst", "NULL", n0_), what); } while (0)

static int write_math(const char* in, const char* out) {
    FILE* f = fopen(in, "rb");
    int32_t count = 0;
    if (!f || fread(&count, 4, 1, f) != 1 || count < 0) return 1;
    float* x = malloc((size_t)count * 24 + 4);
    if (!x || fread(x, 24, (size_t)count, f) != (size_t)count) return 1;
    fclose(f);
    f = fopen(out, "wb");
    if (!f) return 1;
    for (int32_t i = 0; i < count; ++i) {
        const float* a = x + 6 * i;
        const float r = gpd_obst_task_reward(a[0], a[1], a[2], a[3], a[4], a[5]), h = gpd_obst_task_hinge(a[1], a[2], a[4]);
        const int32_t hit = gpd_obst_task_hit(a[1], a[2]);
        if (fwrite(&r, 4, 1, f) != 1 || fwrite(&h, 4, 1, f) != 1 || fwrite(&hit, 4, 1, f) != 1) return 1;
    }
    free(x);
    return fclose(f) != 0;
}

int main(int argc, char** argv) {
    if (argc == 4 && strcmp(argv[1], "math") == 0) return write_math(argv[2], argv[3]);
    defaults();
    const float nan = __builtin_nanf(""), inf = __builtin_inff();
    int32_t size = 0;
    CHECK(gpd_sizeof_obst_task(&size) == 0 && size == (int32_t)sizeof(GpdObstTask) && size == 32, "gpd_sizeof_obst_task: 32 bytes");
    CHECK(gpd_sizeof_obst_task(NULL) == GPD_EINVAL, "gpd_sizeof_obst_task(NULL)");

    /* ---- accepted: one launch of <ACT, EXT, SHARED>; 70 drones, 256 / G per workgroup ---- */
    LAUNCHES("ILi2ELb1ELb1EE", 5u, 7u * 32u, "VEL, every flag, a shared list of 7, 16 rays -> <VEL, EXT, SHARED>, G = 16");
    C.physics_flags = 0; obst_ld = 70; Q.n_rays = 64; row_ld = 80; row_stride = 70 * 80;
    LAUNCHES("ILi2ELb0ELb0EE", 18u, 0u, "VEL, no flag, per-aviary lists, 64 rays -> <VEL, no EXT, lists>, G = 64");
    C.act_type = GPD_ACT_RPM; S.pid = NULL; Q.n_rays = 0; ray_dirs = NULL; row_ld = 16; row_stride = 0; n_obst = 1024;
    LAUNCHES("ILi0ELb1ELb1EE", 1u, 1024u * 32u, "RPM, no state.pid, no rays (NULL ray_dirs), 1024 records, last row only -> <RPM, EXT, SHARED>, G = 1");
    C.act_type = GPD_ACT_RPM; C.physics_flags = 0; S.last_rpm = NULL; Q.n_rays = 1; obst_ld = 131; C.task = GPD_TASK_NONE; target = NULL; C.auto_reset = 0; init_pose = NULL;
    LAUNCHES("ILi0ELb0ELb0EE", 1u, 0u, "RPM, nothing optional, one ray, lists with a pitch above E -> <RPM, no EXT, lists>, G = 1");
    C.act_type = GPD_ACT_PID; Q.n_rays = 5; a_stride = 0; num_steps = 1; Q.hit_terminates = 0;
    LAUNCHES("ILi1ELb1ELb1EE", 3u, 7u * 32u, "PID, a held waypoint, one step, 5 rays -> <PID, EXT, SHARED>, G = 8");
    C.act_type = GPD_ACT_PID; C.physics_flags = GPD_PHYS_GROUND; obst_ld = 70; Q.n_rays = 17; row_ld = 36; row_stride = 70 * 36;
    LAUNCHES("ILi1ELb1ELb0EE", 9u, 0u, "PID, the ground plane alone, lists, 17 rays -> <PID, EXT, lists>, G = 32");
    Q.prox_margin = 0.0f; Q.prox_weight = 0.0f; Q.hit_reward = 0.0f; Q.n_rays = 0; Q.max_range = nan; Q.ray_frame = 9; row_ld = 16; row_stride = 70 * 16;
    LAUNCHES("ILi2ELb1ELb1EE", 1u, 7u * 32u, "no rays: max_range and ray_frame are not read");

    /* ---- GPD_ENOTSUP: what narrows the entry, before any device call ---- */
    C.physics_flags = GPD_PHYS_DW; REFUSED(GPD_ENOTSUP, "downwash", "GPD_PHYS_DW alone");
    C.physics_flags |= GPD_PHYS_DW; REFUSED(GPD_ENOTSUP, "downwash", "GPD_PHYS_DW among the other flags");
    C.drones_per_env = 2; C.num_envs = 35; REFUSED(GPD_ENOTSUP, "drones_per_env", "aviaries of two");
    for (int act = GPD_ACT_RPM; act <= GPD_ACT_DIRECT_RPM; ++act) {
        if (act == GPD_ACT_RPM || act == GPD_ACT_VEL || act == GPD_ACT_PID) continue;
        C.act_type = act; REFUSED(GPD_ENOTSUP, "act_type", "another action type");
    }
    C.task = GPD_TASK_MULTIHOVER; REFUSED(GPD_ENOTSUP, "task", "GPD_TASK_MULTIHOVER");
    S.bad = DEV(20); REFUSED(GPD_ENOTSUP, "state.bad", "the non-finite guard");
    S.act_ring = DEV(21); REFUSED(GPD_ENOTSUP, "state.act_ring", "the action history");
    P.pid_kf = 0.0f; REFUSED(GPD_ENOTSUP, "DSLPID", "VEL on an airframe without DSLPID");

    /* ---- GPD_EINVAL ---- */
    NULL_ARG(gpd_rollout_obst(NULL, &S, &C, &Q, 5, actions, 0, target, init_pose, obst, 7, 1, ray_dirs, rows, 32, 0, reward, terminated, truncated, collided, 0, NULL), "NULL params");
    NULL_ARG(gpd_rollout_obst(&P, NULL, &C, &Q, 5, actions, 0, target, init_pose, obst, 7, 1, ray_dirs, rows, 32, 0, reward, terminated, truncated, collided, 0, NULL), "NULL state");
    NULL_ARG(gpd_rollout_obst(&P, &S, NULL, &Q, 5, actions, 0, target, init_pose, obst, 7, 1, ray_dirs, rows, 32, 0, reward, terminated, truncated, collided, 0, NULL), "NULL cfg");
    NULL_ARG(gpd_rollout_obst(&P, &S, &C, NULL, 5, actions, 0, target, init_pose, obst, 7, 1, ray_dirs, rows, 32, 0, reward, terminated, truncated, collided, 0, NULL), "NULL task");
    actions = NULL; REFUSED(GPD_EINVAL, "NULL", "NULL actions");
    obst = NULL; REFUSED(GPD_EINVAL, "NULL", "NULL obst");
    rows = NULL; REFUSED(GPD_EINVAL, "NULL", "NULL rows");
    reward = NULL; REFUSED(GPD_EINVAL, "NULL", "NULL reward");
    terminated = NULL; REFUSED(GPD_EINVAL, "NULL", "NULL terminated");
    truncated = NULL; REFUSED(GPD_EINVAL, "NULL", "NULL truncated");
    collided = NULL; REFUSED(GPD_EINVAL, "NULL", "NULL collided");
    S.kin = NULL; REFUSED(GPD_EINVAL, "NULL state.kin", "NULL state.kin");
    S.step_counter = NULL; REFUSED(GPD_EINVAL, "NULL state.kin", "NULL state.step_counter");
    S.kin = ODD(DEV(1), 4); REFUSED(GPD_EINVAL, "16-byte", "misaligned state.kin");
    S.ld = 64; REFUSED(GPD_EINVAL, "state.ld", "state.ld < num_envs");
    S.ld = 0; REFUSED(GPD_EINVAL, "state.ld", "state.ld 0");
    S.pid = NULL; REFUSED(GPD_EINVAL, "state.pid", "VEL without state.pid");
    S.last_rpm = NULL; REFUSED(GPD_EINVAL, "last_rpm", "GPD_PHYS_DRAG without state.last_rpm");
    target = NULL; REFUSED(GPD_EINVAL, "target_pos", "a task without target_pos");
    init_pose = NULL; REFUSED(GPD_EINVAL, "init_pose", "auto_reset without init_pose");
    num_steps = 0; REFUSED(GPD_EINVAL, "num_steps", "num_steps 0");
    a_stride = -4; REFUSED(GPD_EINVAL, "strides", "a negative action stride");
    row_stride = -32; REFUSED(GPD_EINVAL, "strides", "a negative row stride");
    env_stride = -1; REFUSED(GPD_EINVAL, "strides", "a negative env stride");
    C.num_envs = 0; REFUSED(GPD_EINVAL, "positive", "num_envs 0");
    C.substeps = 0; REFUSED(GPD_EINVAL, "positive", "substeps 0");
    C.act_type = 9; REFUSED(GPD_EINVAL, "act_type", "unknown act_type");
    C.task = 7; REFUSED(GPD_EINVAL, "task", "unknown task");
    C.physics_flags = 32; REFUSED(GPD_EINVAL, "unknown physics flag", "an unknown physics flag");
    for (int64_t ld = -1; ld <= 69; ld += (ld == 0 ? 2 : (ld == 2 ? 67 : 1))) { obst_ld = ld; REFUSED(GPD_EINVAL, "obst_ld", "obst_ld neither 1 nor >= num_envs"); }
    Q.collision_radius = 0.0f; REFUSED(GPD_EINVAL, "collision_radius", "collision_radius 0");
    Q.collision_radius = -0.1f; REFUSED(GPD_EINVAL, "collision_radius", "collision_radius negative");
    Q.collision_radius = inf; REFUSED(GPD_EINVAL, "collision_radius", "collision_radius infinite");
    Q.collision_radius = nan; REFUSED(GPD_EINVAL, "collision_radius", "collision_radius NaN");
    Q.hit_terminates = 2; REFUSED(GPD_EINVAL, "hit_terminates", "hit_terminates 2");
    Q.hit_terminates = -1; REFUSED(GPD_EINVAL, "hit_terminates", "hit_terminates -1");
    Q.hit_reward = nan; REFUSED(GPD_EINVAL, "hit_reward", "hit_reward NaN");
    Q.hit_reward = -inf; REFUSED(GPD_EINVAL, "hit_reward", "hit_reward -inf");
    Q.prox_margin = -0.1f; REFUSED(GPD_EINVAL, "prox_margin", "prox_margin negative");
    Q.prox_margin = nan; REFUSED(GPD_EINVAL, "prox_margin", "prox_margin NaN");
    Q.prox_weight = -1.0f; REFUSED(GPD_EINVAL, "prox_weight", "prox_weight negative");
    Q.prox_weight = inf; REFUSED(GPD_EINVAL, "prox_weight", "prox_weight infinite");
    ray_dirs = NULL; REFUSED(GPD_EINVAL, "ray_dirs", "rays without ray_dirs");
    Q.ray_frame = 3; REFUSED(GPD_EINVAL, "ray_frame", "unknown ray_frame");
    Q.ray_frame = -1; REFUSED(GPD_EINVAL, "ray_frame", "negative ray_frame");
    Q.max_range = 0.0f; REFUSED(GPD_EINVAL, "max_range", "max_range 0");
    Q.max_range = inf; REFUSED(GPD_EINVAL, "max_range", "max_range infinite");
    Q.max_range = nan; REFUSED(GPD_EINVAL, "max_range", "max_range NaN");
    rows = ODD(DEV(10), 4); REFUSED(GPD_EINVAL, "16-byte", "misaligned rows");
    rows = ODD(DEV(10), 8); REFUSED(GPD_EINVAL, "16-byte", "rows aligned to 8 bytes only");
    row_ld = 28; REFUSED(GPD_EINVAL, "row_ld", "row_ld below 16 + n_rays");
    row_ld = 34; REFUSED(GPD_EINVAL, "row_ld", "row_ld not a multiple of 4");
    row_stride = 70 * 32 + 2; REFUSED(GPD_EINVAL, "row_step_stride", "row_step_stride not a multiple of 4");

    /* ---- GPD_ERANGE ---- */
    n_obst = 0; REFUSED(GPD_ERANGE, "n_obst", "n_obst 0");
    n_obst = -1; REFUSED(GPD_ERANGE, "n_obst", "negative n_obst");
    n_obst = GPD_OBST_MAX + 1; REFUSED(GPD_ERANGE, "n_obst", "n_obst above GPD_OBST_MAX");
    Q.n_rays = -1; REFUSED(GPD_ERANGE, "n_rays", "negative n_rays");
    Q.n_rays = GPD_OBST_MAX_RAYS + 1; row_ld = 84; REFUSED(GPD_ERANGE, "n_rays", "n_rays above GPD_OBST_MAX_RAYS");
    C.num_envs = (1 << 26) + 1; S.ld = (1 << 26) + 64; REFUSED(GPD_ERANGE, "2^26", "more than 2^26 drones");

    /* ---- obst_task_math.inc: the documented corner values ---- */
    CHECK(gpd_obst_task_hit(0.06f, 0.06f) == 0 && gpd_obst_task_hit(0.0599f, 0.06f) == 1 && gpd_obst_task_hit(inf, 0.06f) == 0, "contact is strict; none at +inf");
    CHECK(gpd_obst_task_hinge(inf, 0.06f, 0.5f) == 0.0f && gpd_obst_task_hinge(0.06f, 0.06f, 0.5f) == 0.5f && gpd_obst_task_hinge(1.0f, 0.06f, 0.5f) == 0.0f,
          "the hinge: 0 at +inf and beyond the margin, the margin at contact");
    CHECK(gpd_obst_task_reward(1.25f, inf, 0.06f, -5.0f, 0.5f, 2.0f) == 1.25f && gpd_obst_task_reward(-1.0f, 3.0f, 0.06f, -5.0f, 0.5f, 2.0f) == -1.0f,
          "nothing near: the task's reward, to the bit");
    CHECK(gpd_obst_task_reward(1.0f, 0.0f, 0.25f, -5.0f, 0.5f, 2.0f) == 1.0f - 5.0f - 2.0f * 0.75f, "in contact: hit_reward and the hinge past the margin");
    CHECK(gpd_obst_task_reward(1.0f, 0.0f, 0.25f, -5.0f, 0.5f, 0.0f) == -4.0f && gpd_obst_task_reward(1.0f, 0.5f, 0.25f, -5.0f, 0.0f, 3.0f) == 1.0f,
          "a zero weight or a zero margin: no hinge");
    printf("%d checks failed\n", failed);
    return failed;
}
