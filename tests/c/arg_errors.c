/*
 * What every C-ABI entry refuses, and with which code: from one valid call per entry, one argument is broken at a time, against the
 * host-only sanitized library of tests/test_host_sanitizers.py (tests/stubs/hip_stub.c: nothing is launched).  Prints, for every
 * call the library refuses,
 *     <entry> <case> -> rc <code> | <gpd_last_error()>
 * and nothing for a broken call it accepts (an action type that is out of range for one entry is another entry's valid input).
 * tests/c/arg_errors.expected is the recorded table: the test holds every row's code against it, and every message to
 * "<entry>: ...".  Exit code: valid calls that were refused.  Device pointers are fake (see asan_host.c).  Left out: the RCCL
 * entries, gpd_clock_probe and the debug build's branch of gpd_debug_status.
 */
#include <math.h>
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include "gpd.h"

#define DEV(n) ((void*)(uintptr_t)(0x100000000ull + 0x1000000ull * (n)))
#define OFF4(p) ((void*)((char*)(p) + 4))                   /* a 4-byte offset: not 16-byte aligned */

/* everything a call reads: the case macro saves it, breaks one thing, calls, restores */
static struct All {
    GpdParams P; GpdState S; GpdStepCfg C; GpdPolicy pol; GpdSwarm W; GpdState VS;
    const GpdParams* pP; const GpdState* pS; const GpdStepCfg* pC; const GpdPolicy* ppol; const GpdSwarm* pW; const GpdMrac* pM;
    const GpdState* pVS;
    void* p[16];          /* the entry's pointer arguments; [1] = target_pos and [2] = init_pose wherever an entry has them */
    int64_t s[4];         /* strides / pitches */
    int32_t K, n, i[8];
    float f[8];
} G;
static GpdMrac M;
static const char* entry;
static int (*call)(void);
static int refused_valid;

static void row(const char* what, int rc) {
    if (rc != 0) printf("%s %s -> rc %d | %s\n", entry, what, rc, gpd_last_error());
}
#define X(what, stmt) do { const struct All saved_ = G; stmt; row(what, call()); G = saved_; } while (0)
static void begin(const char* name, int (*fn)(void)) {
    entry = name; call = fn;
    const int rc = call();
    if (rc != 0) { ++refused_valid; fprintf(stderr, "%s: the valid call was refused: rc %d | %s\n", name, rc, gpd_last_error()); }
}

/* ---- what the entries with a GpdStepCfg share: every argument of the common preamble, broken one at a time ---- */
static void cfg_battery(void) {
    char what[64];
    X("params=NULL", G.pP = NULL);
    X("state=NULL", G.pS = NULL);
    X("cfg=NULL", G.pC = NULL);
    X("state.kin=NULL", G.S.kin = NULL);
    X("state.step_counter=NULL", G.S.step_counter = NULL);
    X("state.kin+4", G.S.kin = OFF4(G.S.kin));
    X("state.ld=0", G.S.ld = 0);
    X("state.ld=2^32", G.S.ld = 1ll << 32);
    X("state.ld=N-1", G.S.ld = (int64_t)G.C.num_envs * G.C.drones_per_env - 1);
    X("num_envs=0", G.C.num_envs = 0);
    X("drones_per_env=0", G.C.drones_per_env = 0);
    X("drones_per_env=2", G.C.drones_per_env = 2; G.C.num_envs /= 2);
    X("drones_per_env=128", G.C.drones_per_env = 128; G.C.num_envs /= 128);
    X("drones_per_env=257", G.C.drones_per_env = 257; G.C.num_envs = 8);
    X("substeps=0", G.C.substeps = 0);
    X("substeps=2", G.C.substeps = 2);
    for (int a = -1; a <= 7; ++a) { snprintf(what, sizeof what, "act_type=%d", a); X(what, G.C.act_type = a); }
    for (int t = -1; t <= 3; ++t) { snprintf(what, sizeof what, "task=%d", t); X(what, G.C.task = t); }
    for (uint32_t f = 1; f <= 64; f *= 2) { snprintf(what, sizeof what, "physics_flags=%u", f); X(what, G.C.physics_flags = f); }
    X("physics_flags=0x80000000", G.C.physics_flags = 0x80000000u);
    X("act_type=-1,task=3,physics_flags=32", G.C.act_type = -1; G.C.task = 3; G.C.physics_flags = 32);
    X("task=3,physics_flags=32", G.C.task = 3; G.C.physics_flags = 32);
    X("num_envs=2^26+1", G.C.num_envs = (1 << 26) + 1; G.C.drones_per_env = 1; G.S.ld = (1ll << 26) + 64; G.s[3] = G.S.ld);
    X("act_type=PID,state.pid=NULL", G.C.act_type = GPD_ACT_PID; G.S.pid = NULL);
    X("act_type=VEL,pid_kf=0", G.C.act_type = GPD_ACT_VEL; G.P.pid_kf = 0.0f);
    X("DRAG,state.last_rpm=NULL", G.C.physics_flags = GPD_PHYS_DRAG; G.S.last_rpm = NULL);
    X("task=HOVER,target_pos=NULL", G.C.task = GPD_TASK_HOVER; G.p[1] = NULL);
    X("auto_reset=1", G.C.auto_reset = 1);
    X("auto_reset=1,init_pose=NULL", G.C.auto_reset = 1; G.p[2] = NULL);
    X("lanes_per_wave=48", G.C.lanes_per_wave = 48);
    X("state.dw_force", G.S.dw_force = DEV(47));
    X("num_steps=0", G.K = 0);
    X("strides[0]=-1", G.s[0] = -1);
    X("strides[1]=-1", G.s[1] = -1);
    X("strides[2]=-1", G.s[2] = -1);
}

/* p: 0 action(s) | 1 target_pos | 2 init_pose | 3 obs12 | 4 reward | 5 terminated | 6 truncated | 7 term_obs12 | 8 plant_rows; s: action, obs, env strides */
static int c_step(void) { return gpd_step(G.pP, G.pS, G.pC, G.p[0], G.p[1], G.p[2], G.p[3], G.p[4], G.p[5], G.p[6], G.p[7], NULL); }
static int c_step_sync(void) { return gpd_step_sync(G.pP, G.pS, G.pC, G.p[0], G.p[1], G.p[2], G.p[3], G.p[4], G.p[5], G.p[6], G.p[7], NULL); }
static int c_rollout(void) {
    return gpd_rollout(G.pP, G.pS, G.pC, G.K, G.p[0], G.s[0], G.p[1], G.p[2], G.p[3], G.s[1], G.p[4], G.p[5], G.p[6], G.s[2], G.p[7], NULL);
}
static int c_history(void) {
    return gpd_rollout_history(G.pP, G.pS, G.pC, G.K, G.p[0], G.s[0], G.p[1], G.p[2], G.p[3], G.s[1], G.p[4], G.p[5], G.p[6], G.s[2], NULL);
}
static int c_plant(void) {
    return gpd_rollout_plant(G.pP, G.pS, G.pC, G.K, G.p[0], G.s[0], G.p[1], G.p[2], G.p[3], G.s[1], G.p[4], G.p[5], G.p[6], G.s[2], G.p[7], G.p[8], NULL);
}
/* p: 0 obs12_in | 1, 2 | 3 obs12 .. 7 term_obs12 as above | 8 actions_out | 9 noise | 10 action_std (host) | 11 mean_out */
static int c_policy(void) {
    return gpd_rollout_policy(G.pP, G.pS, G.pC, G.ppol, G.K, G.p[0], G.p[1], G.p[2], G.p[8], G.p[3], G.s[1], G.p[4], G.p[5], G.p[6], G.s[2],
                              G.p[9], G.p[10], G.p[11], G.p[7], NULL);
}
/* p: 0 action | 3 obs12 | 8 vec_out */
static int c_swarm_step(void) { return gpd_swarm_step(G.pP, G.pS, G.pC, G.pW, G.p[0], G.p[3], G.p[8], NULL); }
static int c_swarm_pack(void) { return gpd_swarm_pack(G.pS, G.pW, G.p[3], G.p[8], NULL); }
static int c_swarm_bin(void) { return gpd_swarm_bin(G.pW, NULL); }
static int c_swarm_forces(void) { return gpd_swarm_forces(G.pP, G.pW, G.i[0], NULL); }
/* p: 0 targets | 3 obs12 | 8 plant_rows | 9 mrac_state | 10 counter | 11 rpm_carry; s: 0 target stride, 1 obs stride, 3 mrac_ld */
static int c_rollout_mrac(void) {
    return gpd_rollout_mrac(G.pP, G.pM, G.pS, G.pC, G.p[9], G.p[10], G.s[3], G.p[0], G.s[0], G.p[11], G.p[8], G.p[3], G.s[1], G.K, NULL);
}
/* p: 0 actions | 1 target_pos | 3 obs12 .. 6 truncated | 8 plant_rows | 9 tape | 10 g_obs12 | 11 g_reward | 12 g_kin | 13 g_actions | 14 floats_out */
static int c_tape_floats(void) { return gpd_rollout_tape_floats(G.pC, G.K, G.S.ld, G.p[14]); }
static int c_tape(void) {
    return gpd_rollout_tape(G.pP, G.pS, G.pC, G.K, G.p[0], G.s[0], G.p[1], G.p[3], G.s[1], G.p[4], G.p[5], G.p[6], G.s[2], G.p[8], G.p[9], NULL);
}
static int c_vjp(void) {
    return gpd_rollout_vjp(G.pP, G.pC, G.S.ld, G.K, G.p[0], G.s[0], G.p[1], G.p[8], G.p[9], G.p[10], G.s[1], G.p[11], G.s[2], G.p[12], G.p[13], NULL);
}

static void base(void) {
    memset(&G, 0, sizeof G);
    G.pP = &G.P; G.pS = &G.S; G.pC = &G.C; G.ppol = &G.pol; G.pW = &G.W; G.pM = &M; G.pVS = &G.VS;
    G.P.pid_kf = 3.16e-10f;
    G.S.kin = DEV(1); G.S.step_counter = DEV(2); G.S.last_rpm = DEV(10); G.S.pid = DEV(11); G.S.ld = 4096;
    G.C.num_envs = 4096; G.C.drones_per_env = 1; G.C.substeps = 1; G.C.act_type = GPD_ACT_RPM; G.C.task = GPD_TASK_HOVER;
    G.C.pyb_dt = 1.0f / 240; G.C.ctrl_dt = 1.0f / 240; G.C.inv_ctrl_dt = 240;
    for (int k = 0; k < 9; ++k) G.p[k] = DEV(3 + k);
    G.p[7] = NULL; G.p[8] = NULL;
    G.K = 8; G.s[0] = 4096 * 4; G.s[1] = 4096 * 12; G.s[2] = 4096; G.s[3] = 4096;
}

static void outputs(void) {            /* the outputs an entry names in one message */
    X("action=NULL", G.p[0] = NULL);
    X("obs12=NULL", G.p[3] = NULL);
    X("reward=NULL", G.p[4] = NULL);
    X("terminated=NULL", G.p[5] = NULL);
    X("truncated=NULL", G.p[6] = NULL);
}

static void steps_and_rollouts(void) {
    base(); begin("gpd_step", c_step); cfg_battery(); outputs();
    base(); begin("gpd_step_sync", c_step_sync); cfg_battery(); outputs();
    base(); begin("gpd_rollout", c_rollout); cfg_battery(); outputs();
    base(); G.S.act_ring = DEV(13); G.S.ring_pos = DEV(14); G.S.hist_len = 15;
    begin("gpd_rollout_history", c_history); cfg_battery(); outputs();
    X("state.act_ring=NULL", G.S.act_ring = NULL);
    X("state.ring_pos=NULL", G.S.ring_pos = NULL);
    X("state.hist_len=0", G.S.hist_len = 0);
    X("drones_per_env=65", G.C.drones_per_env = 65; G.C.num_envs = 63);
    X("num_steps=0,state.act_ring=NULL", G.K = 0; G.S.act_ring = NULL);
    X("state.act_ring=NULL,act_type=7", G.S.act_ring = NULL; G.C.act_type = 7);
    base(); G.p[8] = DEV(61);
    begin("gpd_rollout_plant", c_plant); cfg_battery(); outputs();
    X("plant_rows=NULL", G.p[8] = NULL);
    X("plant_rows+4", G.p[8] = OFF4(G.p[8]));
    X("plant_rows=NULL,act_type=7", G.p[8] = NULL; G.C.act_type = 7);
    X("num_steps=0,plant_rows=NULL", G.K = 0; G.p[8] = NULL);
}

static void policy(void) {
    static float action_std[4] = {0.1f, 0.1f, 0.1f, 0.1f};
    base();
    G.pol.w1 = DEV(16); G.pol.b1 = DEV(17); G.pol.w2 = DEV(18); G.pol.b2 = DEV(19); G.pol.w3 = DEV(20); G.pol.b3 = DEV(21);
    G.pol.hidden = 64; G.pol.in_dim = 12; G.p[8] = DEV(22);
    begin("gpd_rollout_policy", c_policy); cfg_battery(); outputs();
    X("noise without action_std", G.p[9] = DEV(29));
    X("action_std without noise", G.p[10] = action_std);
    X("mean_out without noise", G.p[11] = DEV(30));
    X("noise,act_type=VEL", G.p[9] = DEV(29); G.p[10] = action_std; G.C.act_type = GPD_ACT_VEL);
    X("noise,params=NULL", G.p[9] = DEV(29); G.pP = NULL);
    X("policy=NULL", G.ppol = NULL);
    X("policy.w1=NULL", G.pol.w1 = NULL);
    X("policy.b3=NULL", G.pol.b3 = NULL);
    X("policy.hidden=32", G.pol.hidden = 32);
    X("policy.activation=2", G.pol.activation = 2);
    X("policy.hidden=32,physics_flags=32", G.pol.hidden = 32; G.C.physics_flags = 32);
    X("policy.in_dim=13", G.pol.in_dim = 13);
    X("policy.in_dim=13,ring", G.pol.in_dim = 13; G.S.act_ring = DEV(13); G.S.ring_pos = DEV(14); G.S.hist_len = 15);
    X("policy.in_dim=72,state.ring_pos=NULL", G.pol.in_dim = 72; G.S.act_ring = DEV(13); G.S.hist_len = 15);
    X("hist_len=18", G.pol.in_dim = 12 + 18 * 4; G.S.act_ring = DEV(13); G.S.ring_pos = DEV(14); G.S.hist_len = 18);
    X("hist_len=21,act_type=ONE_D_RPM", G.pol.in_dim = 12 + 21; G.C.act_type = GPD_ACT_ONE_D_RPM; G.S.act_ring = DEV(13); G.S.ring_pos = DEV(14); G.S.hist_len = 21);
    X("state.act_ring without ring_pos", G.S.act_ring = DEV(13); G.S.hist_len = 15);
    X("state.act_ring without hist_len", G.S.act_ring = DEV(13); G.S.ring_pos = DEV(14));
    X("drones_per_env=2,act_type=7", G.C.drones_per_env = 2; G.C.num_envs = 2048; G.C.act_type = 7);
    X("act_type=5,task=3", G.C.act_type = 5; G.C.task = 3);
}

static void swarm_base(void) {
    base();
    GpdSwarm* w = &G.W;
    w->world_size = 1; w->rank = 0; w->own_count = 65536; w->nx = w->ny = 32; w->nz = 1; w->cell = 10.5f; w->x0 = w->y0 = -170.0f; w->zbin = 1.0f;
    w->meta_rows = 256; w->slab = w->n_rows = 65792;
    w->pos4 = DEV(40); w->bin_pos = DEV(41); w->cell_count = DEV(42); w->cell_start = DEV(43); w->order = DEV(44); w->visit_out = DEV(45);
    w->slot_key = DEV(46); w->dw_force = DEV(47); w->slot_of = DEV(48); w->pos_sorted = DEV(49); w->pair_list = DEV(50); w->pair_nb = DEV(51);
    w->list_ok = DEV(52); w->list_cap = 48; w->list_delta = 0.245f; w->drift = DEV(53); w->total_drones = 65536; w->list_adapt = 1;
    G.C.num_envs = 65536; G.C.task = GPD_TASK_NONE; G.C.act_type = GPD_ACT_RAW_RPM; G.C.physics_flags = 31; G.S.ld = 65536; G.S.dw_force = DEV(47);
}
static void swarm_battery(void) {
    X("swarm=NULL", G.pW = NULL);
    X("world_size=0", G.W.world_size = 0);
    X("world_size=257", G.W.world_size = 257);
    X("rank=-1", G.W.rank = -1);
    X("rank=1", G.W.rank = 1);
    X("meta_rows=0", G.W.meta_rows = 0);
    X("own_count=-1", G.W.own_count = -1);
    X("own_count=slab", G.W.own_count = G.W.slab);
    X("meta_rows=255", G.W.meta_rows = 255);
    X("slot_of=NULL", G.W.slot_of = NULL);
    X("pos_sorted=NULL", G.W.pos_sorted = NULL);
    X("world_size=2 with slot_of", G.W.world_size = 2; G.W.n_rows = 2 * G.W.slab);
    X("n_rows=slab+1", G.W.n_rows = G.W.slab + 1);
    X("n_rows=2^26+256", G.W.slab = G.W.n_rows = (1 << 26) + 256);
    X("pos4=NULL", G.W.pos4 = NULL);
    X("bin_pos=NULL", G.W.bin_pos = NULL);
    X("drift=NULL", G.W.drift = NULL);
    X("total_drones=0", G.W.total_drones = 0);
    X("total_drones=n_rows+1", G.W.total_drones = G.W.n_rows + 1);
    X("cell_count=NULL", G.W.cell_count = NULL);
    X("cell_start=NULL", G.W.cell_start = NULL);
    X("order=NULL", G.W.order = NULL);
    X("slot_key=NULL", G.W.slot_key = NULL);
    X("visit=order", G.W.visit = G.W.order);
    X("visit=visit_out", G.W.visit = G.W.visit_out);
    X("cell=5", G.W.cell = 5.0f);
    X("cell=NaN", G.W.cell = NAN);
    X("nz=0", G.W.nz = 0);
    X("nz=257", G.W.nz = 257);
    X("nz=2,zbin=0", G.W.nz = 2; G.W.zbin = 0.0f);
    X("nx=2", G.W.nx = 2);
    X("nx=ny=256,nz=2", G.W.nx = G.W.ny = 256; G.W.nz = 2);
    X("dw_force=NULL", G.W.dw_force = NULL);
}
static void one_world(void) {
    swarm_base(); begin("gpd_swarm_step", c_swarm_step); cfg_battery(); swarm_battery();
    X("action=NULL", G.p[0] = NULL);
    X("obs12=NULL", G.p[3] = NULL);
    X("num_envs=own_count-1", G.C.num_envs = G.W.own_count - 1);
    X("state.ld=num_envs-1", G.S.ld = G.C.num_envs - 1);
    X("swarm=NULL,state.kin=NULL", G.pW = NULL; G.S.kin = NULL);
    X("substeps=2,physics_flags=32", G.C.substeps = 2; G.C.physics_flags = 32);
    swarm_base(); begin("gpd_swarm_pack", c_swarm_pack); swarm_battery();
    X("state=NULL", G.pS = NULL);
    X("state.kin=NULL", G.S.kin = NULL);
    X("state.kin+4", G.S.kin = OFF4(G.S.kin));
    X("state.ld=0", G.S.ld = 0);
    X("state.ld=2^32", G.S.ld = 1ll << 32);
    X("state.ld=own_count-1", G.S.ld = G.W.own_count - 1);
    X("vec_out without obs12", G.p[8] = DEV(23); G.p[3] = NULL);
    X("state.kin+4,swarm=NULL", G.S.kin = OFF4(G.S.kin); G.pW = NULL);
    swarm_base(); begin("gpd_swarm_bin", c_swarm_bin); swarm_battery();
    swarm_base(); begin("gpd_swarm_forces", c_swarm_forces); swarm_battery();
    X("params=NULL", G.pP = NULL);
    X("pair_nb=NULL", G.W.pair_nb = NULL);
    X("list_ok=NULL", G.W.list_ok = NULL);
    X("list_cap=2", G.W.list_cap = 2);
    X("list_cap=65536", G.W.list_cap = 65536);
    X("list_delta=-1", G.W.list_delta = -1.0f);
    X("list_delta=NaN", G.W.list_delta = NAN);
    X("n_rows=2^26", G.W.slab = G.W.n_rows = 1 << 26);
    X("pair_list=NULL,pair_nb=NULL", G.W.pair_list = NULL; G.W.pair_nb = NULL);     /* (accepted: no lists) */
}

/* p: 0 kin | 1 visit_order | 2 cell_count | 3 cell_start | 4 order | 5 sorted_xyzc | 6 dw_out | 7 vec_obs12 | 8 vec_out; i: nx ny nz; f: cell zbin */
static int c_downwash(void) {
    return gpd_downwash_global(G.pP, G.p[0], G.s[0], G.n, G.f[0], -170.0f, -170.0f, G.i[0], G.i[1], 0.0f, G.f[1], G.i[2], G.p[1], G.p[2], G.p[3],
                               G.p[4], G.p[5], G.p[6], G.pVS, G.p[7], G.p[8], NULL);
}
static void downwash(void) {
    base();
    G.p[0] = DEV(1); G.p[1] = NULL; G.p[2] = DEV(30); G.p[3] = DEV(31); G.p[4] = DEV(32); G.p[5] = DEV(33); G.p[6] = DEV(34); G.p[7] = NULL; G.p[8] = NULL;
    G.s[0] = 65536; G.n = 65536; G.f[0] = 10.5f; G.f[1] = 1.0f; G.i[0] = G.i[1] = 32; G.i[2] = 1;
    G.VS = G.S; G.VS.ld = 65536;
    begin("gpd_downwash_global", c_downwash);
    X("params=NULL", G.pP = NULL);
    X("kin=NULL", G.p[0] = NULL);
    X("cell_count=NULL", G.p[2] = NULL);
    X("cell_start=NULL", G.p[3] = NULL);
    X("order=NULL", G.p[4] = NULL);
    X("sorted_xyzc=NULL", G.p[5] = NULL);
    X("dw_out=NULL", G.p[6] = NULL);
    X("n=0", G.n = 0);
    X("ld=n-1", G.s[0] = G.n - 1);
    X("kin+4", G.p[0] = OFF4(G.p[0]));
    X("visit_order=order", G.p[1] = G.p[4]);
    X("cell=9", G.f[0] = 9.0f);
    X("nz=0", G.i[2] = 0);
    X("nz=257", G.i[2] = 257);
    X("nz=2,zbin=0", G.i[2] = 2; G.f[1] = 0.0f);
    X("nx=2", G.i[0] = 2);
    X("ny=2", G.i[1] = 2);
    X("nx=ny=256,nz=2", G.i[0] = G.i[1] = 256; G.i[2] = 2);
    X("vec_out without vec_state", G.p[8] = DEV(23); G.p[7] = DEV(6); G.pVS = NULL);
    X("vec_out,vec_state.kin=NULL", G.p[8] = DEV(23); G.p[7] = DEV(6); G.VS.kin = NULL);
    X("vec_out without vec_obs12", G.p[8] = DEV(23));
    X("vec_out,vec_state.ld=n-1", G.p[8] = DEV(23); G.p[7] = DEV(6); G.VS.ld = G.n - 1);
}

/* p: 0 pos4 | 1 visit_order | 2 cell_count | 3 cell_start | 4 order | 5 sorted_xyzc | 6 nbr_count | 7 nbr_idx | 8 nbr_rel | 9 adjacency;
 * i: n_rows, query_first, query_count, k, drones_per_env; f: radius, cell, x0, y0, x1, y1 */
static int c_neighbors(void) {
    return gpd_neighbors(G.p[0], G.i[0], G.i[1], G.i[2], G.f[0], G.i[3], G.i[4], G.f[1], G.f[2], G.f[3], G.f[4], G.f[5], G.p[1], G.p[2], G.p[3], G.p[4],
                         G.p[5], G.p[6], G.p[7], G.p[8], G.p[9], NULL);
}
static void neighbors(void) {
    base();
    memset(G.p, 0, sizeof G.p);
    G.p[0] = DEV(40); G.p[2] = DEV(42); G.p[3] = DEV(43); G.p[4] = DEV(44); G.p[5] = DEV(49); G.p[6] = DEV(54); G.p[7] = DEV(55); G.p[8] = DEV(56);
    G.i[0] = 65536; G.i[1] = 0; G.i[2] = 65536; G.i[3] = 5; G.i[4] = 0;
    G.f[0] = 2.0f; G.f[1] = 0.0f; G.f[2] = G.f[3] = -170.0f; G.f[4] = G.f[5] = 170.0f;
    begin("gpd_neighbors", c_neighbors);
    X("pos4=NULL", G.p[0] = NULL);
    X("nbr_count=NULL", G.p[6] = NULL);
    X("n_rows=0", G.i[0] = 0);
    X("k=0", G.i[3] = 0);
    X("k=33", G.i[3] = 33);
    X("radius=0", G.f[0] = 0.0f);
    X("radius=inf", G.f[0] = INFINITY);
    X("radius=NaN", G.f[0] = NAN);
    X("query_first=-1", G.i[1] = -1);
    X("query_count=0", G.i[2] = 0);
    X("query_first=1", G.i[1] = 1);
    X("pos4+4", G.p[0] = OFF4(G.p[0]));
    X("nbr_rel+4", G.p[8] = OFF4(G.p[8]));
    X("drones_per_env=1", G.i[4] = 1);
    X("drones_per_env=257", G.i[4] = 257);
    X("drones_per_env=-2", G.i[4] = -2);
    X("adjacency,drones_per_env=0", G.p[9] = DEV(57));
    X("drones_per_env=3", G.i[4] = 3);
    X("drones_per_env=8,query_first=4", G.i[4] = 8; G.i[1] = 4; G.i[2] = 64);
    X("drones_per_env=8,query_count=60", G.i[4] = 8; G.i[2] = 60);
    X("cell_count=NULL", G.p[2] = NULL);
    X("cell_start=NULL", G.p[3] = NULL);
    X("order=NULL", G.p[4] = NULL);
    X("sorted_xyzc=NULL", G.p[5] = NULL);
    X("visit_order=order", G.p[1] = G.p[4]);
    X("sorted_xyzc+4", G.p[5] = OFF4(G.p[5]));
    X("x0=NaN", G.f[2] = NAN);
    X("y1=inf", G.f[5] = INFINITY);
    X("x1<x0", G.f[4] = -171.0f);
    X("y1<y0", G.f[5] = -171.0f);
    X("cell=-1", G.f[1] = -1.0f);
    X("cell=inf", G.f[1] = INFINITY);
}

/* p: 0 actions | 3 obs12 | 8 obs_full; i: n_drones, drones_per_env, act_dim; s: 0 action, 1 obs, 2 full strides */
static int c_hist_rows(void) { return gpd_hist_rows(G.pS, G.i[0], G.i[1], G.i[2], G.p[3], G.p[8], NULL); }
static int c_full_obs(void) { return gpd_full_obs(G.pS, G.K, G.i[0], G.i[1], G.i[2], G.p[3], G.s[1], G.p[0], G.s[0], G.p[8], G.s[2], NULL); }
static void hist_base(void) {
    base();
    G.S.act_ring = DEV(13); G.S.ring_pos = DEV(14); G.S.hist_len = 15;
    G.i[0] = 4096; G.i[1] = 1; G.i[2] = 4; G.p[8] = DEV(15); G.s[2] = 4096 * 72;
}
static void hist_battery(void) {
    X("state=NULL", G.pS = NULL);
    X("state.act_ring=NULL", G.S.act_ring = NULL);
    X("state.ring_pos=NULL", G.S.ring_pos = NULL);
    X("state.hist_len=0", G.S.hist_len = 0);
    X("n_drones=0", G.i[0] = 0);
    X("drones_per_env=0", G.i[1] = 0);
    X("drones_per_env=5", G.i[1] = 5);
    X("act_dim=0", G.i[2] = 0);
    X("act_dim=5", G.i[2] = 5);
    X("n_drones=2^26", G.i[0] = 1 << 26);
    X("hist_len=4000", G.S.hist_len = 4000);
    X("obs12=NULL", G.p[3] = NULL);
}
static void history_rows(void) {
    hist_base(); begin("gpd_hist_rows", c_hist_rows); hist_battery();
    X("obs_full=NULL", G.p[8] = NULL);
    hist_base(); begin("gpd_full_obs", c_full_obs); hist_battery();
    X("actions=NULL", G.p[0] = NULL);
    X("num_steps=0", G.K = 0);
    X("num_steps=65536", G.K = 65536);
    X("obs_step_stride=-1", G.s[1] = -1);
    X("action_step_stride=-1", G.s[0] = -1);
    X("full_step_stride=-1", G.s[2] = -1);
    X("obs_full=NULL,obs12=NULL", G.p[8] = NULL; G.p[3] = NULL);                 /* (accepted: the ring update alone) */
}

/* p: 2 init_pose | 3 obs12 | 8 mask / state20 */
static int c_reset(void) { return gpd_reset(G.pS, G.p[2], G.i[0], G.p[8], G.C.num_envs, G.C.drones_per_env, G.i[1], G.p[3], NULL); }
static int c_state_vectors(void) { return gpd_state_vectors(G.pS, G.p[3], G.p[8], G.n, NULL); }
static void state_battery(void) {
    X("state=NULL", G.pS = NULL);
    X("state.kin=NULL", G.S.kin = NULL);
    X("state.step_counter=NULL", G.S.step_counter = NULL);
    X("state.kin+4", G.S.kin = OFF4(G.S.kin));
    X("state.ld=0", G.S.ld = 0);
    X("state.ld=2^32", G.S.ld = 1ll << 32);
    X("state.ld=4095", G.S.ld = 4095);
    X("obs12=NULL", G.p[3] = NULL);
}
static void reset_and_vectors(void) {
    base(); begin("gpd_reset", c_reset); state_battery();
    X("init_pose=NULL", G.p[2] = NULL);
    X("num_envs=0", G.C.num_envs = 0);
    X("drones_per_env=0", G.C.drones_per_env = 0);
    X("state.ld=N-1,drones_per_env=2", G.C.drones_per_env = 2; G.S.ld = 8191);
    base(); G.n = 4096; G.p[8] = DEV(23);
    begin("gpd_state_vectors", c_state_vectors); state_battery();
    X("state20=NULL", G.p[8] = NULL);
    X("n=0", G.n = 0);
}

/* p: 0 pid | 1 cur_pos | 2 cur_quat | 3 cur_vel | 4 target_pos | 5 rpm | 6 cur_ang_vel | 9 mrac_state | 10 counter | 11 mask; s[0] = ld; f[0] = ctrl_dt */
static int c_pid(void) { return gpd_pid(G.pP, G.p[0], G.s[0], G.f[0], G.p[1], G.p[2], G.p[3], G.p[4], NULL, NULL, NULL, G.p[5], NULL, NULL, G.n, NULL); }
static int c_pid_sync(void) { return gpd_pid_sync(G.pP, G.p[0], G.s[0], G.f[0], G.p[1], G.p[2], G.p[3], G.p[4], NULL, NULL, NULL, G.p[5], NULL, NULL, G.n, NULL); }
static int c_mrac(void) {
    return gpd_mrac(G.pM, G.p[9], G.p[10], G.s[0], G.f[0], G.p[1], G.p[2], G.p[3], G.p[6], G.p[4], NULL, NULL, NULL, G.p[5], NULL, NULL, G.n, NULL);
}
static int c_mrac_reset(void) { return gpd_mrac_reset(G.p[9], G.p[10], G.s[0], G.pM, G.p[11], G.n, G.i[0], NULL); }
static void ctrl_base(void) {
    base();
    G.p[0] = DEV(11); G.p[1] = DEV(24); G.p[2] = DEV(25); G.p[3] = DEV(26); G.p[4] = DEV(27); G.p[5] = DEV(28); G.p[6] = DEV(62);
    G.p[9] = DEV(57); G.p[10] = DEV(58); G.p[11] = NULL;
    G.s[0] = 4096; G.n = 4096; G.f[0] = 1.0f / 240;
}
static void ctrl_battery(void) {
    X("cur_pos=NULL", G.p[1] = NULL);
    X("cur_quat=NULL", G.p[2] = NULL);
    X("cur_vel=NULL", G.p[3] = NULL);
    X("target_pos=NULL", G.p[4] = NULL);
    X("rpm=NULL", G.p[5] = NULL);
    X("n=0", G.n = 0);
    X("ld=n-1", G.s[0] = G.n - 1);
    X("n=2^26+1", G.n = (1 << 26) + 1; G.s[0] = G.n);
}
static void controllers(void) {
    ctrl_base(); begin("gpd_pid", c_pid); ctrl_battery();
    X("params=NULL", G.pP = NULL);
    X("pid=NULL", G.p[0] = NULL);
    X("pid_kf=0", G.P.pid_kf = 0.0f);
    ctrl_base(); begin("gpd_pid_sync", c_pid_sync); ctrl_battery();
    X("params=NULL", G.pP = NULL);
    X("pid=NULL", G.p[0] = NULL);
    X("pid_kf=0", G.P.pid_kf = 0.0f);
    ctrl_base(); begin("gpd_mrac", c_mrac); ctrl_battery();
    X("mrac=NULL", G.pM = NULL);
    X("mrac_state=NULL", G.p[9] = NULL);
    X("counter=NULL", G.p[10] = NULL);
    X("cur_ang_vel=NULL", G.p[6] = NULL);
    X("ctrl_dt=0", G.f[0] = 0.0f);
    X("ctrl_dt=NaN", G.f[0] = NAN);
    X("cur_quat+4", G.p[2] = OFF4(G.p[2]));
    X("rpm+4", G.p[5] = OFF4(G.p[5]));
    ctrl_base(); begin("gpd_mrac_reset", c_mrac_reset);
    X("mrac_state=NULL", G.p[9] = NULL);
    X("counter=NULL", G.p[10] = NULL);
    X("restore_gains,mrac=NULL", G.i[0] = 1; G.pM = NULL);
    X("mrac=NULL", G.pM = NULL);                                                   /* (accepted without restore_gains) */
    X("n=0", G.n = 0);
    X("ld=n-1", G.s[0] = G.n - 1);
    X("n=2^26+1", G.n = (1 << 26) + 1; G.s[0] = G.n);
    int32_t size = 0;
    entry = "gpd_sizeof_mrac";
    if (gpd_sizeof_mrac(&size) != 0 || size != (int32_t)sizeof(GpdMrac)) ++refused_valid;
    row("size_out=NULL", gpd_sizeof_mrac(NULL));
}

static void rollout_mrac(void) {
    base();
    G.C.task = GPD_TASK_NONE; G.C.act_type = GPD_ACT_RAW_RPM;
    G.p[0] = DEV(59); G.p[3] = DEV(6); G.p[8] = DEV(61); G.p[9] = DEV(57); G.p[10] = DEV(58); G.p[11] = DEV(60);
    G.s[0] = 4096 * 12; G.s[1] = 4096 * 12; G.s[3] = 4096;
    begin("gpd_rollout_mrac", c_rollout_mrac); cfg_battery();
    X("mrac=NULL", G.pM = NULL);
    X("mrac_state=NULL", G.p[9] = NULL);
    X("counter=NULL", G.p[10] = NULL);
    X("targets=NULL", G.p[0] = NULL);
    X("rpm_carry=NULL", G.p[11] = NULL);
    X("obs12=NULL", G.p[3] = NULL);
    X("plant_rows=NULL", G.p[8] = NULL);                                           /* (accepted: no plant table) */
    X("mrac_ld=N-1", G.s[3] = 4095);
    X("target_step_stride=12N-4", G.s[0] = 12 * 4096 - 4);
    X("obs_step_stride=12N-4", G.s[1] = 12 * 4096 - 4);
    X("target_step_stride=12N+2", G.s[0] = 12 * 4096 + 2);
    X("obs_step_stride=12N+2", G.s[1] = 12 * 4096 + 2);
    X("targets+4", G.p[0] = OFF4(G.p[0]));
    X("rpm_carry+4", G.p[11] = OFF4(G.p[11]));
    X("obs12+4", G.p[3] = OFF4(G.p[3]));
    X("plant_rows+4", G.p[8] = OFF4(G.p[8]));
    X("ctrl_dt=0", G.C.ctrl_dt = 0.0f);
    X("pyb_dt=0", G.C.pyb_dt = 0.0f);
    X("drones_per_env=2,physics_flags=32", G.C.drones_per_env = 2; G.C.num_envs = 2048; G.C.physics_flags = 32);
    X("drones_per_env=2,num_steps=0", G.C.drones_per_env = 2; G.C.num_envs = 2048; G.K = 0);
    X("act_type=0,state.ld=N-1", G.C.act_type = 0; G.S.ld = 4095);
    X("state.kin+4,mrac_state=NULL", G.S.kin = OFF4(G.S.kin); G.p[9] = NULL);
}

static int c_plant_derive(void) { return gpd_plant_derive(G.pP, G.p[0], G.p[1], G.C.num_envs, G.C.drones_per_env, G.S.ld, G.p[8], NULL); }
static void plant_derive(void) {
    base(); G.p[0] = DEV(63); G.p[1] = NULL; G.p[8] = DEV(61);
    begin("gpd_plant_derive", c_plant_derive);
    X("nominal=NULL", G.pP = NULL);
    X("scales=NULL", G.p[0] = NULL);
    X("rows=NULL", G.p[8] = NULL);
    X("num_envs=0", G.C.num_envs = 0);
    X("drones_per_env=0", G.C.drones_per_env = 0);
    X("ld=N-1", G.S.ld = 4095);
    X("num_envs=2^26+1", G.C.num_envs = (1 << 26) + 1; G.S.ld = (1ll << 26) + 64);
    X("rows+4", G.p[8] = OFF4(G.p[8]));
}

static void differentiable(void) {
    static int64_t floats;
    base(); G.p[14] = &floats;
    begin("gpd_rollout_tape_floats", c_tape_floats); cfg_battery();
    X("floats_out=NULL", G.p[14] = NULL);
    X("num_steps=2^31-1,ld=2^32-1", G.K = INT32_MAX; G.S.ld = 0xffffffffll);
    X("act_type=PID,physics_flags=32", G.C.act_type = GPD_ACT_PID; G.C.physics_flags = 32);
    X("drones_per_env=2,task=3", G.C.drones_per_env = 2; G.C.num_envs = 2048; G.C.task = 3);
    base(); G.p[8] = DEV(61); G.p[9] = DEV(64);
    begin("gpd_rollout_tape", c_tape); cfg_battery(); outputs();
    X("tape=NULL", G.p[9] = NULL);
    X("tape+4", G.p[9] = OFF4(G.p[9]));
    X("plant_rows+4", G.p[8] = OFF4(G.p[8]));
    X("plant_rows=NULL", G.p[8] = NULL);                                           /* (accepted: no plant table) */
    X("act_type=PID,physics_flags=32", G.C.act_type = GPD_ACT_PID; G.C.physics_flags = 32);
    X("drones_per_env=2,task=3", G.C.drones_per_env = 2; G.C.num_envs = 2048; G.C.task = 3);
    X("strides[0]=-1,num_steps=0", G.s[0] = -1; G.K = 0);
    base(); G.p[8] = DEV(61); G.p[9] = DEV(64); G.p[10] = DEV(65); G.p[11] = DEV(66); G.p[12] = DEV(67); G.p[13] = DEV(68);
    begin("gpd_rollout_vjp", c_vjp); cfg_battery();
    X("actions=NULL", G.p[0] = NULL);
    X("tape=NULL", G.p[9] = NULL);
    X("g_kin=NULL", G.p[12] = NULL);
    X("g_actions=NULL", G.p[13] = NULL);
    X("g_obs12=NULL,g_reward=NULL", G.p[10] = NULL; G.p[11] = NULL);              /* (accepted: no cotangent of that output) */
    X("tape+4", G.p[9] = OFF4(G.p[9]));
    X("g_kin+4", G.p[12] = OFF4(G.p[12]));
    X("plant_rows+4", G.p[8] = OFF4(G.p[8]));
    X("g_actions+4", G.p[13] = OFF4(G.p[13]));
    X("act_type=PID,physics_flags=32", G.C.act_type = GPD_ACT_PID; G.C.physics_flags = 32);
    X("drones_per_env=2,task=3", G.C.drones_per_env = 2; G.C.num_envs = 2048; G.C.task = 3);
    X("strides[0]=-1,num_steps=0", G.s[0] = -1; G.K = 0);
}

int main(void) {
    steps_and_rollouts();
    policy();
    one_world();
    downwash();
    neighbors();
    history_rows();
    reset_and_vectors();
    controllers();
    rollout_mrac();
    plant_derive();
    differentiable();
    uint32_t dbg[4];
    entry = "gpd_debug_status";
    row("release build", gpd_debug_status(dbg, 0, NULL));
    if (refused_valid) fprintf(stderr, "%d valid calls were refused\n", refused_valid);
    return refused_valid;
}
