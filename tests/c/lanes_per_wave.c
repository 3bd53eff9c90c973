/*
 * GpdStepCfg.lanes_per_wave on the host side: 0 means 64, the values 16 / 32 / 64 size the single-step grid ((256 / 64) lanes_per_wave
 * drones per workgroup), a rollout of more than one step and a multi-drone aviary ignore it, and every other value is refused with
 * GPD_EINVAL and the library's message before anything is launched -- by each of the five entries that read the field.  Against the
 * host-only sanitized library and the launch stub (tests/helpers/host_lib.py, tests/stubs/hip_stub.c); run by
 * tests/test_host_sanitizers.py.  Prints one line per check; exit code = failed checks.
 */
#include "host_check.h"

static GpdParams P;
static GpdState S;
static GpdStepCfg C;

static int step(void) { return gpd_step(&P, &S, &C, DEV(3), DEV(4), DEV(5), DEV(6), DEV(7), DEV(8), DEV(9), NULL, NULL); }
static int step_sync(void) { return gpd_step_sync(&P, &S, &C, DEV(3), DEV(4), DEV(5), DEV(6), DEV(7), DEV(8), DEV(9), NULL, NULL); }
static int rollout_k(int K) {
    return gpd_rollout(&P, &S, &C, K, DEV(3), (int64_t)C.num_envs * C.drones_per_env * 4, DEV(4), DEV(5), DEV(6),
                       (int64_t)C.num_envs * C.drones_per_env * 12, DEV(7), DEV(8), DEV(9), C.num_envs, NULL, NULL);
}
static int rollout(void) { return rollout_k(8); }
static int history(void) {
    return gpd_rollout_history(&P, &S, &C, 8, DEV(3), (int64_t)C.num_envs * 4, DEV(4), DEV(5), DEV(6), (int64_t)C.num_envs * 12, DEV(7), DEV(8), DEV(9),
                               C.num_envs, NULL);
}
static int plant(void) {
    return gpd_rollout_plant(&P, &S, &C, 8, DEV(3), (int64_t)C.num_envs * 4, DEV(4), DEV(5), DEV(6), (int64_t)C.num_envs * 12, DEV(7), DEV(8), DEV(9),
                             C.num_envs, NULL, DEV(61), NULL);
}

int main(void) {
    static const struct { const char* name; int (*call)(void); } entries[] = {
        {"gpd_step", step}, {"gpd_step_sync", step_sync}, {"gpd_rollout", rollout}, {"gpd_rollout_history", history}, {"gpd_rollout_plant", plant}};
    static const int bad[] = {8, 48, -1, 1, 63, 65, 128};
    char what[96];
    unsigned last[7];
    P.pid_kf = 3.16e-10f;
    S.kin = DEV(1); S.step_counter = DEV(2); S.last_rpm = DEV(10); S.ld = 4160;
    S.act_ring = DEV(13); S.ring_pos = DEV(14); S.hist_len = 15;
    C.num_envs = 4100; C.drones_per_env = 1; C.substeps = 1; C.act_type = GPD_ACT_RPM; C.task = GPD_TASK_HOVER;
    C.pyb_dt = 1.0f / 240; C.ctrl_dt = 1.0f / 240; C.inv_ctrl_dt = 240;

    for (size_t e = 0; e < sizeof entries / sizeof entries[0]; ++e) {
        for (size_t b = 0; b < sizeof bad / sizeof bad[0]; ++b) {
            const int n0 = hipstub_launches();
            C.lanes_per_wave = bad[b];
            snprintf(what, sizeof what, "%s refuses lanes_per_wave = %d", entries[e].name, bad[b]);
            CHECK(refused(entries[e].call(), GPD_EINVAL, entries[e].name, "lanes_per_wave must be 0, 16, 32 or 64", n0), what);
        }
        static const int good[] = {0, 16, 32, 64};
        for (size_t g = 0; g < sizeof good / sizeof good[0]; ++g) {
            const int n0 = hipstub_launches();
            C.lanes_per_wave = good[g];
            snprintf(what, sizeof what, "%s accepts lanes_per_wave = %d", entries[e].name, good[g]);
            CHECK(entries[e].call() == 0 && hipstub_launches() == n0 + 1, what);
        }
    }
    S.act_ring = NULL; S.ring_pos = NULL; S.hist_len = 0;

    /* the single-step grid: ceil(N / (4 lanes_per_wave)) workgroups of 256 lanes; 0 is 64 */
    static const struct { int lanes; unsigned blocks; } grid[] = {{0, 17}, {64, 17}, {32, 33}, {16, 65}};
    for (size_t g = 0; g < sizeof grid / sizeof grid[0]; ++g) {
        C.lanes_per_wave = grid[g].lanes;
        snprintf(what, sizeof what, "4100 drones, lanes_per_wave = %d: %u workgroups of gpd_step_kernel", grid[g].lanes, grid[g].blocks);
        const int rc = step();
        hipstub_last(last);
        CHECK(rc == 0 && KERNEL("gpd_step_kernel") && last[0] == grid[g].blocks && last[3] == 256, what);
        snprintf(what, sizeof what, "... and of a one-step gpd_rollout, which is routed to the same kernel (lanes_per_wave = %d)", grid[g].lanes);
        const int rc1 = rollout_k(1);
        hipstub_last(last);
        CHECK(rc1 == 0 && KERNEL("gpd_step_kernel") && last[0] == grid[g].blocks && last[3] == 256, what);
        snprintf(what, sizeof what, "a rollout of 8 steps keeps its 256 drones per workgroup (lanes_per_wave = %d)", grid[g].lanes);
        const int rc8 = rollout();
        hipstub_last(last);
        CHECK(rc8 == 0 && KERNEL("gpd_rollout1_kernel") && last[0] == 17 && last[3] == 256, what);
    }
    /* whole aviaries per workgroup: the field does not enter the packing (7 aviaries of 33 drones = 231 lanes) */
    C.drones_per_env = 33; C.num_envs = 9; S.ld = 320; C.task = GPD_TASK_MULTIHOVER;
    for (size_t g = 0; g < sizeof grid / sizeof grid[0]; ++g) {
        C.lanes_per_wave = grid[g].lanes;
        snprintf(what, sizeof what, "9 aviaries of 33 drones, lanes_per_wave = %d: two workgroups", grid[g].lanes);
        const int rc = step();
        hipstub_last(last);
        CHECK(rc == 0 && KERNEL("gpd_step_kernel") && last[0] == 2 && last[3] == 256, what);
    }
    printf("%d checks failed\n", failed);
    return failed;
}
