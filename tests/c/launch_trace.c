/*
 * Which kernel serves which call: drives the launching entries of include/gpd.h over the shapes at which their launch paths decide
 * something, against the host-only library of tests/test_host_sanitizers.py (tests/stubs/hip_stub.c names every launch), and prints
 *     <entry> <case> -> <kernel symbol> <grid.x> <block.x> <dynamic LDS bytes>
 * once per launch, or `<entry> <case> -> rc <code>` for a call the library refuses (`-> nothing` if an accepted call launched
 * nothing).  The test holds the trace's invariants; the trace itself is what a change of a launch path is compared by, before
 * against after.  Device pointers are fake (see asan_host.c).
 */
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include "gpd.h"

void hipstub_on_launch(void (*f)(const char*, const unsigned[7]));

#define DEV(n) ((void*)(uintptr_t)(0x100000000ull + 0x1000000ull * (n)))
static const char* entry;
static char what[160];
static int launched;

static void on_launch(const char* kernel, const unsigned g[7]) {
    ++launched;
    printf("%s %s -> %s %u %u %u\n", entry, what, kernel, g[0], g[3], g[6]);
}
static void done(int rc) {
    if (rc != 0) printf("%s %s -> rc %d\n", entry, what, rc);
    else if (!launched) printf("%s %s -> nothing\n", entry, what);
    launched = 0;
}

static GpdParams P;
static GpdState S;
static GpdStepCfg C;

static void steps_and_rollouts(void) {
    static const int Ks[] = {1, 20, 64}, Ds[] = {1, 2, 3, 8, 64, 100}, subs[] = {1, 8}, envs[] = {1, 4096};
    static const uint32_t flags[] = {0, 4, 7, 24, 31};
    static const char* const names[] = {"gpd_step", "gpd_rollout", "gpd_rollout_history", "gpd_rollout_plant"};
    for (int which = 0; which < 4; ++which)
        for (int ki = 0; ki < (which == 0 ? 1 : 3); ++ki)
            for (int term = 0; term < (which == 2 ? 1 : 2); ++term)
                for (int act = GPD_ACT_RPM; act <= GPD_ACT_DIRECT_RPM; ++act)
                    for (int fi = 0; fi < 5; ++fi)
                        for (int di = 0; di < 6; ++di)
                            for (int si = 0; si < 2; ++si)
                                for (int ei = 0; ei < 2 + (which != 0); ++ei) {
                                    /* (the extra size: more than 2^17 drones, for the shape that stores its observations differently below that) */
                                    const int big = ei == 2, K = which == 0 ? 1 : Ks[ki], E = big ? 262144 : envs[ei];
                                    if (big && (K != 64 || Ds[di] != 1)) continue;
                                    const int64_t N = (int64_t)E * Ds[di];
                                    entry = names[which];
                                    snprintf(what, sizeof what, "K=%d,term=%d,act=%d,flags=%u,D=%d,sub=%d,E=%d", K, term, act, flags[fi], Ds[di], subs[si], E);
                                    C.num_envs = E; C.drones_per_env = Ds[di]; C.act_type = act; C.substeps = subs[si]; C.physics_flags = flags[fi];
                                    S.ld = (N + 63) / 64 * 64;
                                    S.act_ring = which == 2 ? DEV(13) : NULL; S.ring_pos = which == 2 ? DEV(14) : NULL; S.hist_len = which == 2 ? 15 : 0;
                                    float* const to = term ? DEV(12) : NULL;
                                    const int64_t as = N * 4, os = N * 12;
                                    if (which == 0) done(gpd_step(&P, &S, &C, DEV(3), DEV(4), DEV(5), DEV(6), DEV(7), DEV(8), DEV(9), to, NULL));
                                    else if (which == 1) done(gpd_rollout(&P, &S, &C, K, DEV(3), as, DEV(4), DEV(5), DEV(6), os, DEV(7), DEV(8), DEV(9), E, to, NULL));
                                    else if (which == 2) done(gpd_rollout_history(&P, &S, &C, K, DEV(3), as, DEV(4), DEV(5), DEV(6), os, DEV(7), DEV(8), DEV(9), E, NULL));
                                    else done(gpd_rollout_plant(&P, &S, &C, K, DEV(3), as, DEV(4), DEV(5), DEV(6), os, DEV(7), DEV(8), DEV(9), E, to, DEV(61), NULL));
                                }
    S.act_ring = NULL; S.ring_pos = NULL; S.hist_len = 0;
}

static void policies(void) {
    static const float action_std[4] = {0.1f, 0.1f, 0.1f, 0.1f};
    GpdPolicy pol;
    memset(&pol, 0, sizeof pol);
    pol.w1 = DEV(16); pol.b1 = DEV(17); pol.w2 = DEV(18); pol.b2 = DEV(19); pol.w3 = DEV(20); pol.b3 = DEV(21); pol.hidden = 64;
    C.num_envs = 4096; C.drones_per_env = 1; C.substeps = 1; C.physics_flags = 0; S.ld = 4096;
    S.act_ring = DEV(13); S.ring_pos = DEV(14); S.hist_len = 15;
    entry = "gpd_rollout_policy";
    for (int act = GPD_ACT_RPM; act <= GPD_ACT_ONE_D_PID; ++act)
        for (int hist = 0; hist < 2; ++hist)
            for (int relu = 0; relu < 2; ++relu)
                for (int noise = 0; noise < 2; ++noise) {
                    const int A = (act == GPD_ACT_RPM || act == GPD_ACT_VEL) ? 4 : (act == GPD_ACT_PID ? 3 : 1);
                    C.act_type = act; pol.in_dim = 12 + (hist ? S.hist_len * A : 0); pol.activation = relu;
                    snprintf(what, sizeof what, "act=%d,in_dim=%d,activation=%d,noise=%d", act, pol.in_dim, relu, noise);
                    done(gpd_rollout_policy(&P, &S, &C, &pol, 8, DEV(6), DEV(4), DEV(5), DEV(22), DEV(6), 4096 * 12, DEV(7), DEV(8), DEV(9), 4096,
                                            noise ? DEV(29) : NULL, noise ? action_std : NULL, NULL, NULL, NULL));
                }
    S.act_ring = NULL; S.ring_pos = NULL; S.hist_len = 0;
}

static void one_world(void) {
    GpdSwarm W;
    memset(&W, 0, sizeof W);
    W.world_size = 1; W.rank = 0; W.own_count = 65536; W.nx = W.ny = 32; W.nz = 1; W.cell = 10.5f; W.x0 = W.y0 = -170.0f; W.zbin = 1.0f;
    W.pos4 = DEV(40); W.bin_pos = DEV(41); W.cell_count = DEV(42); W.cell_start = DEV(43); W.order = DEV(44); W.visit_out = DEV(45);
    W.slot_key = DEV(46); W.dw_force = DEV(47); W.slot_of = DEV(48); W.pos_sorted = DEV(49); W.pair_nb = DEV(51); W.list_ok = DEV(52);
    W.list_cap = 48; W.list_delta = 0.245f; W.drift = DEV(53); W.total_drones = 65536; W.list_adapt = 1;
    C.num_envs = 65536; C.drones_per_env = 1; C.substeps = 1; C.task = GPD_TASK_NONE; C.physics_flags = 31; C.auto_reset = 0;
    S.ld = 65536; S.dw_force = DEV(47);
    entry = "gpd_swarm_step";
    for (int meta = 256; meta <= 1280; meta += 1024)          /* world_size * meta_rows on both sides of 1024 */
        for (int a = 0; a < 3; ++a) {
            C.act_type = a == 0 ? GPD_ACT_RPM : (a == 1 ? GPD_ACT_RAW_RPM : GPD_ACT_DIRECT_RPM);
            W.meta_rows = meta; W.slab = 65536 + meta; W.n_rows = W.slab;
            snprintf(what, sizeof what, "act=%d,meta_rows=%d", C.act_type, meta);
            done(gpd_swarm_step(&P, &S, &C, &W, DEV(3), DEV(6), DEV(23), NULL));
        }
    W.meta_rows = 256; W.slab = W.n_rows = 65792;
    for (int nz = 1; nz <= 8; nz += 7) {                        /* 1024 and 8192 keys: on both sides of 4096 */
        W.nz = nz;
        entry = "gpd_swarm_bin";
        snprintf(what, sizeof what, "keys=%d", 32 * 32 * nz);
        done(gpd_swarm_bin(&W, NULL));
        entry = "gpd_downwash_global";
        for (int vec = 0; vec < 2; ++vec) {
            snprintf(what, sizeof what, "keys=%d,vec_out=%d", 32 * 32 * nz, vec);
            done(gpd_downwash_global(&P, DEV(1), 65536, 65536, 10.5f, -170.0f, -170.0f, 32, 32, 0.0f, 1.0f, nz, NULL, DEV(30), DEV(31), DEV(32), DEV(33),
                                     DEV(34), vec ? &S : NULL, vec ? DEV(6) : NULL, vec ? DEV(23) : NULL, NULL));
        }
    }
    W.nz = 1;
    entry = "gpd_swarm_forces";
    for (int mode = 0; mode < 3; ++mode) {
        W.pair_list = mode ? DEV(50) : NULL;
        snprintf(what, sizeof what, "lists=%s", mode == 0 ? "none" : (mode == 1 ? "build" : "replay"));
        done(gpd_swarm_forces(&P, &W, mode == 1, NULL));
    }
    S.dw_force = NULL;
    static const int ks[] = {1, 4, 5, 8, 9, 16, 17, 32};
    entry = "gpd_neighbors";
    for (int ki = 0; ki < 8; ++ki)
        for (int shape = 0; shape < 4; ++shape) {              /* one world over a box of 2500 or 28 224 cells (4096: the sort's threshold); aviaries */
            const int D = shape < 2 ? 0 : (shape == 2 ? 2 : 256);
            const float half = shape == 0 ? 50.0f : 170.0f;
            snprintf(what, sizeof what, "k=%d,D=%d,box=%g", ks[ki], D, 2.0 * half);
            done(gpd_neighbors(DEV(40), 65536, 0, 65536, 2.0f, ks[ki], D, 0.0f, -half, -half, half, half, NULL, DEV(42), DEV(43), DEV(44), DEV(49),
                               DEV(54), DEV(55), DEV(56), NULL, NULL));
        }
}

static void mrac(void) {
    static GpdMrac M;
    static const uint32_t flags[] = {0, 3, 7};                 /* (7 holds the downwash: refused) */
    C.num_envs = 4096; C.drones_per_env = 1; C.substeps = 1; C.task = GPD_TASK_NONE; C.auto_reset = 0; C.act_type = GPD_ACT_RAW_RPM; S.ld = 4096;
    entry = "gpd_rollout_mrac";
    for (int fi = 0; fi < 3; ++fi)
        for (int plant = 0; plant < 2; ++plant) {
            C.physics_flags = flags[fi];
            snprintf(what, sizeof what, "flags=%u,plant=%d", flags[fi], plant);
            done(gpd_rollout_mrac(&P, &M, &S, &C, DEV(57), DEV(58), 4096, DEV(59), 0, DEV(60), plant ? DEV(61) : NULL, DEV(6), 0, 8, NULL));
        }
}

/* the differentiable rollout: both act widths, with and without drag (EXT) and a plant table */
static void differentiable(void) {
    static const int acts[] = {GPD_ACT_RPM, GPD_ACT_ONE_D_RPM, GPD_ACT_RAW_RPM, GPD_ACT_DIRECT_RPM};
    C.num_envs = 4096; C.drones_per_env = 1; C.substeps = 1; C.auto_reset = 0; S.ld = 4096;
    for (int vjp = 0; vjp < 2; ++vjp)
        for (int ai = 0; ai < 4; ++ai)
            for (int drag = 0; drag < 2; ++drag)
                for (int plant = 0; plant < 2; ++plant)
                    for (int task = GPD_TASK_NONE; task <= GPD_TASK_HOVER; ++task) {
                        const int A = acts[ai] == GPD_ACT_ONE_D_RPM ? 1 : 4;
                        C.act_type = acts[ai]; C.physics_flags = drag ? GPD_PHYS_DRAG : 0; C.task = task;
                        entry = vjp ? "gpd_rollout_vjp" : "gpd_rollout_tape";
                        snprintf(what, sizeof what, "act=%d,flags=%u,plant=%d,task=%d", C.act_type, C.physics_flags, plant, task);
                        const float* const rows = plant ? DEV(61) : NULL;
                        if (vjp) done(gpd_rollout_vjp(&P, &C, S.ld, 8, DEV(3), 4096 * A, DEV(4), rows, DEV(64), DEV(65), 4096 * 12, DEV(66), 4096, DEV(67), DEV(68), NULL));
                        else done(gpd_rollout_tape(&P, &S, &C, 8, DEV(3), 4096 * A, DEV(4), DEV(6), 4096 * 12, DEV(7), DEV(8), DEV(9), 4096, rows, DEV(64), NULL));
                    }
    C.task = GPD_TASK_HOVER; C.auto_reset = 1; C.physics_flags = 0;
}

/* the entries with one launch path each, on both sides of what their grids depend on */
static void small_entries(void) {
    static GpdMrac M;
    static const int ns[] = {1, 64, 257, 4096};
    C.act_type = GPD_ACT_RPM; C.physics_flags = 0; C.drones_per_env = 1; C.substeps = 1;
    for (int ni = 0; ni < 4; ++ni) {
        const int n = ns[ni];
        S.ld = (n + 63) / 64 * 64; C.num_envs = n;
        snprintf(what, sizeof what, "n=%d", n);
        entry = "gpd_reset"; done(gpd_reset(&S, DEV(5), 0, NULL, n, 1, 1, DEV(6), NULL));
        entry = "gpd_state_vectors"; done(gpd_state_vectors(&S, DEV(6), DEV(23), n, NULL));
        entry = "gpd_pid"; done(gpd_pid(&P, DEV(11), S.ld, 1.0f / 240, DEV(24), DEV(25), DEV(26), DEV(27), NULL, NULL, NULL, DEV(28), NULL, NULL, n, NULL));
        entry = "gpd_pid_sync"; done(gpd_pid_sync(&P, DEV(11), S.ld, 1.0f / 240, DEV(24), DEV(25), DEV(26), DEV(27), NULL, NULL, NULL, DEV(28), NULL, NULL, n, NULL));
        entry = "gpd_step_sync"; done(gpd_step_sync(&P, &S, &C, DEV(3), DEV(4), DEV(5), DEV(6), DEV(7), DEV(8), DEV(9), NULL, NULL));
        entry = "gpd_mrac"; done(gpd_mrac(&M, DEV(57), DEV(58), S.ld, 1.0f / 240, DEV(24), DEV(25), DEV(26), DEV(62), DEV(27), NULL, NULL, NULL, DEV(28), NULL, NULL, n, NULL));
        entry = "gpd_plant_derive"; done(gpd_plant_derive(&P, DEV(63), NULL, n, 1, S.ld, DEV(61), NULL));
        entry = "gpd_mrac_reset";
        for (int restore = 0; restore < 2; ++restore) {
            snprintf(what, sizeof what, "n=%d,restore_gains=%d", n, restore);
            done(gpd_mrac_reset(DEV(57), DEV(58), S.ld, &M, NULL, n, restore, NULL));
        }
    }
    entry = "gpd_plant_derive"; snprintf(what, sizeof what, "E=100,D=3"); done(gpd_plant_derive(&P, DEV(63), DEV(69), 100, 3, 320, DEV(61), NULL));
    entry = "gpd_reset"; done(gpd_reset(&S, DEV(5), 1, DEV(69), 100, 3, 0, NULL, NULL));
    /* the history rows: rows per workgroup follow the row length (12 + hist_len * act_dim floats against 48 KiB of LDS) */
    static const int hs[] = {15, 120, 1000};
    S.act_ring = DEV(13); S.ring_pos = DEV(14);
    for (int hi = 0; hi < 3; ++hi)
        for (int A = 1; A <= 4; A += 3)
            for (int D = 1; D <= 2; ++D) {
                S.hist_len = hs[hi];
                snprintf(what, sizeof what, "hist_len=%d,act_dim=%d,D=%d", hs[hi], A, D);
                const int64_t W = 12 + hs[hi] * A;
                entry = "gpd_hist_rows"; done(gpd_hist_rows(&S, 4096, D, A, DEV(6), DEV(15), NULL));
                entry = "gpd_full_obs";
                for (int K = 8; K <= 2000; K += 1992)
                    for (int full = 0; full < 2; ++full) {
                        snprintf(what, sizeof what, "hist_len=%d,act_dim=%d,D=%d,K=%d,obs_full=%d", hs[hi], A, D, K, full);
                        done(gpd_full_obs(&S, K, 4096, D, A, DEV(6), 4096 * 12, DEV(3), 4096 * A, full ? DEV(15) : NULL, 4096 * W, NULL));
                    }
            }
    S.act_ring = NULL; S.ring_pos = NULL; S.hist_len = 0;
    /* gpd_swarm_pack: one lane per row of the rank's slab */
    GpdSwarm W;
    memset(&W, 0, sizeof W);
    W.world_size = 2; W.nx = W.ny = 32; W.nz = 1; W.cell = 10.5f; W.zbin = 1.0f; W.pos4 = DEV(40); W.bin_pos = DEV(41); W.drift = DEV(53);
    entry = "gpd_swarm_pack";
    for (int rank = 0; rank < 2; ++rank)
        for (int own = 1000; own <= 65536; own += 64536) {
            W.rank = rank; W.own_count = own; W.meta_rows = (own + 255) / 256; W.slab = own + W.meta_rows; W.n_rows = 2 * W.slab; W.total_drones = 2 * own;
            S.ld = 65536;
            snprintf(what, sizeof what, "rank=%d,own_count=%d", rank, own);
            done(gpd_swarm_pack(&S, &W, DEV(6), rank ? DEV(23) : NULL, NULL));
        }
}

int main(void) {
    hipstub_on_launch(on_launch);
    P.pid_kf = 3.16e-10f;
    S.kin = DEV(1); S.step_counter = DEV(2); S.last_rpm = DEV(10); S.pid = DEV(11);
    C.task = GPD_TASK_HOVER; C.pyb_dt = 1.0f / 240; C.ctrl_dt = 1.0f / 240; C.inv_ctrl_dt = 240; C.auto_reset = 1;
    steps_and_rollouts();
    policies();
    one_world();
    mrac();
    C.task = GPD_TASK_HOVER; C.auto_reset = 1;
    differentiable();
    small_entries();
    return 0;
}
