// gpd_common.inc — the MI355X (gfx950 / CDNA4) hot path of the vectorised quadrotor simulator: what its five translation units share.
//
// One wavefront lane per drone.  A lane loads its 13 kinematic floats from the structure-of-arrays
// state (four planes: three of float4 and one of float => a wave's load of a plane is one coalesced 1 KiB /
// 256 B transaction), keeps them in VGPRs across all physics sub-steps -- and, in a rollout, across all K env
// steps of the launch -- and stores them back once; the per-airframe constants arrive BY VALUE in the
// kernel-argument segment and therefore live in SGPRs (they are wave-uniform).  No MFMA: there is no
// dense contraction on this path.
//
// Kernels (DESIGN.md section 3):
//   gpd_step_kernel      one env step per launch                                  (gpd_step)
//   gpd_rollout1_kernel  K env steps per launch, aviaries of 1, 2, 4 .. 64 drones (gpd_rollout)
//   gpd_rollout_kernel   K env steps per launch, compute waves + a store wave     (gpd_rollout: other aviary
//                        sizes, terminal observations)
//   gpd_hist_rows_kernel / gpd_hist_push_kernel  action ring + full KIN rows      (gpd_hist_rows, gpd_full_obs)
//   dwg_*_kernel         downwash inside one aviary of any size, grid binning     (gpd_downwash_global)
//   gpd_reset_kernel, gpd_pid_kernel, gpd_state20_kernel
//
// What one env step fuses (env_step; reference = utiasDSL/gym-pybullet-drones, gym_pybullet_drones/...):
//   action -> RPM                      envs/BaseRLAviary.py:187-239, envs/CtrlAviary.py:140
//   DSLPID position + attitude loops   control/DSLPIDControl.py:187-259
//   S x { forces/torques, Euler eqn, semi-implicit Euler, exact quaternion update }
//                                      envs/BaseAviary.py:831-892
//   ground effect / drag / downwash    envs/BaseAviary.py:739-743, 771-774, 798-804 (inside the
//                                      explicit integrator, SURVEY.md App. A.4)
//   quat -> rpy, world body rates      envs/BaseAviary.py:517-519, 873
//   obs12 = pos|rpy|vel|ang_v          envs/BaseRLAviary.py:314
//   reward / terminated / truncated    envs/HoverAviary.py:68-117, envs/MultiHoverAviary.py:75-130
//   step counter, same-step auto-reset envs/BaseAviary.py:382, 451-477
//
// Arithmetic: fp32, NO -ffast-math, FP contraction OFF with every fused multiply-add written as fmaf() (a drone's
// trajectory is bit-identical in every kernel variant, batch size and lane).  At N = 65 536 the kernels are
// bound by the instruction issue of one wave per SIMD, so the hot functions are written for few instructions
// at <= 2 ulp instead of calling the branchy IEEE/OCML versions:
//   1/x, sqrt, 1/sqrt      v_rcp_f32 / v_sqrt_f32 / v_rsq_f32 (1 ulp)
//   quaternion exponential cos(t) and sin(t)/t as even polynomials in t^2 (no sqrt, no division, no
//                          range reduction; |t| <= 1 rad per sub-step, exact OCML path beyond)
//   atan2 / asin           one odd minimax polynomial on [0,1] (abs err 7e-8) + octant fix-up
//   rotor thrusts          carried as deviations from the hover thrust (no cancellation near hover)
// Build: hipcc -O3 -std=c++17 --offload-arch=gfx950 -ffp-contract=off -fno-slp-vectorize -mllvm -amdgpu-sched-strategy=max-ilp -fPIC -shared
#pragma once
#include <hip/hip_runtime.h>
#include <rccl/rccl.h>      // types and enums only: the library itself is resolved at run time (dlopen), see Rccl below
#include <dlfcn.h>

#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <type_traits>

#include "gpd.h"

namespace {

// Floating-point contraction is OFF for the whole file and every fused multiply-add is written out as fmaf():
// which a*b+c pairs get fused would otherwise depend on the code around each inlined copy of a function, and the
// same drone would round differently in the single-step kernel, the rollout kernel and the multi-drone variants.
// With explicit FMAs a drone's trajectory is bit-identical in every kernel variant, batch size and lane.
#pragma clang fp contract(off)

#ifndef GPD_BLOCK
#define GPD_BLOCK 256
#endif
constexpr int kBlock = GPD_BLOCK;   // 256 = 4 wavefronts; one workgroup per CU fills all 4 SIMDs

// A run-time value as a template argument: a launch path hands Const<value>{} to a generic lambda, which names the kernel with
// decltype(arg)::value -- every kernel is launched from ONE place, and only the combinations some call site passes are instantiated.
template <auto V> using Const = std::integral_constant<decltype(V), V>;

}  // namespace
// The library is built from FIVE translation units over this header -- step_rollout.hip, policy.hip, swarm.hip, abi.hip, mrac.hip -- because
// the kernels want different instruction schedulers (-amdgpu-sched-strategy: max-ilp fills the packed-fp32 hazards of the physics; the
// default strategy is 10 % faster on the MFMA / activation mix of the policy kernel, A/B in round 2) and because one 3 800-line unit
// took three minutes to compile.  The last-error string is shared (defined in abi.hip).
std::string& gpd_detail_last_error();
// The DSLPID variants of the policy kernel are instantiated in step_rollout.hip (max-ilp scheduler).  Compiled in the policy unit
// (default scheduler) at commit 7333ea5, the VEL variant returned `truncated` = 1 and a task reward for every aviary whatever the
// configuration said.  ROOT CAUSE (found in the assembly, DESIGN.md section 3.7; reproduced again in round 4, scratch/exp_r04/
// README.md): a register-allocation defect of hipcc (ROCm 7.2.0, AMD clang 22.0.0git roc-7.2.0), not undefined behaviour in this source -- the entry
// block loads GpdStepCfg.task .. init_per_env with `s_load_dwordx8 s[48:55], s[0:1], 0x19c`, the next block loads sixteen
// GpdParams words with `s_load_dwordx16 s[36:51], s[0:1], 0x18` OVER the first four while they are live, and only then is "the
// configuration" saved with `v_writelane_b32 v164, s48..s55, 29..36`: the step loop reloads prop_y[1..3] and gnd_eff_coeff as
// task / xy_bound / z_bound / tilt_bound.  It depends on how the allocator splits that one live range, i.e. on everything
// around it: today's source compiles clean in BOTH units under BOTH schedulers.  Fences: tests/isa_spill_check.py (backward SGPR
// liveness over every kernel of both units: a kernel-argument tuple that is spilled whole after part of it was overwritten),
// tests/test_kernel_isa.py (also builds the policy unit WITH these variants -- GPD_PID_POLICY_IN_POLICY_TU -- under both
// schedulers and checks them), the bitwise cross-kernel tests with every argument word scrambled (tests/test_gpu_policy.py), and
// tests/test_gpu_policy.py::test_vel_policy_kernel_is_right_under_both_schedulers (the variant library, built on the GPU box).
struct GpdPolicyLaunch {
    const GpdParams* params; const GpdState* state; const GpdStepCfg* cfg; const void* span; const GpdPolicy* policy;
    const float* obs12_in; const float* target_pos; const float* init_pose; float* actions_out; float* obs12; float* reward;
    uint8_t* terminated; uint8_t* truncated; void* stream; unsigned grid; int hist; float* term_obs12;
};
void gpd_detail_launch_policy_pid(const GpdPolicyLaunch& a);
// How a `*_sync` entry (gpd_step_sync, gpd_pid_sync) learns that its launch is done.  hipStreamSynchronize costs a barrier packet
// behind the kernel, its completion signal and the runtime's wait: 12.4 us for an EMPTY kernel on MI355X against 7.6 us when the
// kernel's last act is a system-scope release store of a sequence number into page-locked memory the host spins on
// (scratch/exp_r06/sync_latency.hip, profiles/r06_sync_latency_microbench.txt).  A launch with ONE active wave -- one wave issues
// its memory operations in order, so "this wave's stores are released" is "the call's results are visible" -- gets the word of the
// calling thread (`begin`) and ends with `signal_done`; `wait` spins on it and takes hipStreamSynchronize for every other shape
// (`used` false), when no word could be allocated, when the word stays silent for 2 ms (work queued ahead on the stream, a
// capture in progress), and on every 256th call (the runtime retires its bookkeeping of the launches at a synchronisation).
// Defined in abi.hip.
struct GpdDone { uint32_t* flag; uint32_t seq; bool used; };
GpdDone gpd_detail_done_begin();
int gpd_detail_done_wait(const GpdDone& d, void* stream, const char* who);
__device__ __forceinline__ void signal_done(uint32_t* __restrict__ flag, const uint32_t seq, const bool first_lane) {
    if (__builtin_expect(flag != nullptr, 0)) {          // (wave-uniform; NULL for every caller but the *_sync entries: one scalar compare)
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "");
        if (first_lane) __hip_atomic_store(flag, seq, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_SYSTEM);
    }
}
// ------------------------------------------------------------------------------------------------
// Debug-bounds build (-DGPD_DEBUG_BOUNDS; `_native.build(debug=True)` -> libgpd_debug.so, used through GPD_LIB): the kernels
// check every index they READ FROM MEMORY before they address with it -- ring positions, sort keys, slot -> row entries, wake-list
// entries and counts -- record the first violation in a device word (code, workgroup, offending value, number of violations) and
// clamp the index so that the launch stays inside its buffers; `gpd_debug_status` reads the record.  The reference has nothing of
// the kind (SURVEY.md section 5: no sanitizer, no race or bounds checks; its numpy indexing raises IndexError instead).  A
// release build compiles the checks away and `gpd_debug_status` returns GPD_ENOTSUP.  Every unit whose kernels carry checks
// (step_rollout.hip, swarm.hip, policy.hip) keeps a record of its own and exports a reader (GPD_DBG_READER); gpd_debug_status merges them.
// ------------------------------------------------------------------------------------------------
int gpd_detail_dbg_read_step(unsigned int out[4], int reset, void* stream);
int gpd_detail_dbg_read_swarm(unsigned int out[4], int reset, void* stream);
int gpd_detail_dbg_read_policy(unsigned int out[4], int reset, void* stream);
#if defined(GPD_DEBUG_BOUNDS)
static __device__ unsigned int gpd_dbg_word[4];
#define GPD_DBG_READER(name)                                                                                          \
    int name(unsigned int out[4], int reset, void* stream) {                                                          \
        hipStream_t st = static_cast<hipStream_t>(stream);                                                            \
        hipError_t e = hipMemcpyFromSymbolAsync(out, HIP_SYMBOL(gpd_dbg_word), 16, 0, hipMemcpyDeviceToHost, st);     \
        if (e == hipSuccess) e = hipStreamSynchronize(st);                                                            \
        if (e == hipSuccess && reset) {                                                                               \
            const unsigned int zero[4] = {0, 0, 0, 0};                                                                \
            e = hipMemcpyToSymbolAsync(HIP_SYMBOL(gpd_dbg_word), zero, 16, 0, hipMemcpyHostToDevice, st);             \
            if (e == hipSuccess) e = hipStreamSynchronize(st);                                                        \
        }                                                                                                             \
        return static_cast<int>(e);                                                                                   \
    }
#define GPD_DBG(cond, code, val)                                                                  \
    do {                                                                                          \
        if (!(cond)) {                                                                            \
            if (atomicCAS(&gpd_dbg_word[0], 0u, static_cast<unsigned int>(code)) == 0u) {         \
                gpd_dbg_word[1] = blockIdx.x;                                                     \
                gpd_dbg_word[2] = static_cast<unsigned int>(val);                                 \
            }                                                                                     \
            atomicAdd(&gpd_dbg_word[3], 1u);                                                      \
        }                                                                                         \
    } while (0)
#define GPD_DBG_CLAMP(v, lo, hi) ((v) < (lo) ? (lo) : ((v) > (hi) ? (hi) : (v)))
#else
#define GPD_DBG(cond, code, val) do { } while (0)
#define GPD_DBG_CLAMP(v, lo, hi) (v)
#define GPD_DBG_READER(name) int name(unsigned int out[4], int, void*) { out[0] = out[1] = out[2] = out[3] = 0; return 0; }
#endif
namespace {
#define g_last_error gpd_detail_last_error()

int fail(int code, const char* msg) {
    g_last_error = msg;
    return code;
}

int hip_fail(hipError_t e, const char* where) {
    g_last_error = std::string(where) + ": " + hipGetErrorString(e);
    return static_cast<int>(e);
}

// What the kernels assume about GpdState.kin beyond "not NULL" (include/gpd.h, the plane layout): the planes are moved with
// 16-byte vector accesses, so kin must be 16-byte aligned (ld is counted in floats, so every plane then is -- the planes start
// at multiples of 4 ld floats), and the pitch travels to the kernels as a 32-bit argument.  nullptr = fine.
[[maybe_unused]] bool misaligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15u) != 0; }

[[maybe_unused]] const char* state_layout_problem(const GpdState* s) {
    if (misaligned16(s->kin)) return "state.kin must be 16-byte aligned (the planes are read and written as float4)";
    if (s->ld <= 0 || s->ld > 0xffffffffLL) return "state.ld must be in 1 .. 2^32 - 1 (floats)";
    return nullptr;
}

// ------------------------------------------------------------------------------------------------
// The host side of an entry: what it refuses, its launch, `launched`.  An entry holds a Refuse with its own name -- every message
// reads "<entry>: <reason>", built only when the entry refuses (an accepted call allocates nothing) -- and runs the shared checks
// below in the order ITS codes need: what narrows an entry (GPD_ENOTSUP) stays in the entry, in front of the shared check it must
// win against.  tests/c/arg_errors.expected is the recorded table of every entry's refusals.
// ------------------------------------------------------------------------------------------------
struct Refuse {
    const char* who;
    int operator()(int code, const char* msg, const char* more = "") const { return fail(code, (std::string(who) + ": " + msg + more).c_str()); }
};

// after an entry's last launch: 0, or the runtime's error under "<who><what>"
[[maybe_unused]] int launched(const char* who, const char* what = " launch") {
    const hipError_t e = hipGetLastError();
    return e == hipSuccess ? 0 : hip_fail(e, (std::string(who) + what).c_str());
}
[[maybe_unused]] unsigned blocks_for(int64_t n, int64_t per) { return static_cast<unsigned>((n + per - 1) / per); }

[[maybe_unused]] int check_state(Refuse bad, const GpdState* s) {
    if (!s->kin || !s->step_counter) return bad(GPD_EINVAL, "NULL state.kin/step_counter");
    const char* const why = state_layout_problem(s);
    return why ? bad(GPD_EINVAL, why) : 0;
}
[[maybe_unused]] int check_steps(Refuse bad, int32_t num_steps, int64_t stride0 = 0, int64_t stride1 = 0, int64_t stride2 = 0) {
    if (num_steps <= 0) return bad(GPD_EINVAL, "num_steps must be positive");
    return (stride0 < 0 || stride1 < 0 || stride2 < 0) ? bad(GPD_EINVAL, "strides must be non-negative") : 0;
}
[[maybe_unused]] int check_ranges(Refuse bad, const GpdStepCfg* cfg) {
    if (cfg->act_type < GPD_ACT_RPM || cfg->act_type > GPD_ACT_DIRECT_RPM) return bad(GPD_EINVAL, "unknown act_type");
    return (cfg->task < GPD_TASK_NONE || cfg->task > GPD_TASK_MULTIHOVER) ? bad(GPD_EINVAL, "unknown task") : 0;
}
[[maybe_unused]] int check_positive(Refuse bad, const GpdStepCfg* cfg) {
    const bool ok = cfg->num_envs > 0 && cfg->drones_per_env > 0 && cfg->substeps > 0;
    return ok ? 0 : bad(GPD_EINVAL, "num_envs, drones_per_env and substeps must be positive");
}
[[maybe_unused]] int check_flags(Refuse bad, const GpdStepCfg* cfg) { return (cfg->physics_flags & ~31u) ? bad(GPD_EINVAL, "unknown physics flag") : 0; }
// N drones in rows of `ld` floats; `pitch`: what the caller knows `ld` as ("ld" where an entry takes the pitch without the state)
[[maybe_unused]] int check_extent(Refuse bad, int64_t N, int64_t ld, const char* pitch = "state.ld") {
    if (ld < N) return bad(GPD_EINVAL, pitch, " < num_envs*drones_per_env");
    return N > (1LL << 26) ? bad(GPD_ERANGE, "more than 2^26 drones per launch (32-bit byte offsets)") : 0;
}
// what a configuration needs of the optional pointers (`state`: NULL where the entry has none)
[[maybe_unused]] int check_needs(Refuse bad, const GpdParams* params, const GpdState* state, const GpdStepCfg* cfg, const float* target_pos,
                                 const float* init_pose) {
    const bool pid = cfg->act_type == GPD_ACT_PID || cfg->act_type == GPD_ACT_VEL || cfg->act_type == GPD_ACT_ONE_D_PID;
    if (pid && state && !state->pid) return bad(GPD_EINVAL, "PID action type needs state.pid");
    if (pid && params->pid_kf <= 0.0f) return bad(GPD_ENOTSUP, "no DSLPID controller for this airframe (CF2X/CF2P only)");
    if ((cfg->physics_flags & GPD_PHYS_DRAG) && state && !state->last_rpm) return bad(GPD_EINVAL, "GPD_PHYS_DRAG needs state.last_rpm");
    if (cfg->task != GPD_TASK_NONE && !target_pos) return bad(GPD_EINVAL, "task needs target_pos");
    return (cfg->auto_reset && !init_pose) ? bad(GPD_EINVAL, "auto_reset needs init_pose") : 0;
}
// GPD_TASK_NONE never uses the target: hand the kernel a readable dummy so that its load section is branch-free
[[maybe_unused]] void dummy_target(GpdStepCfg& c, const float*& target_pos, const float* readable) {
    if (c.task == GPD_TASK_NONE) { target_pos = readable; c.target_per_env = 0; }
}
// any physics flag / a plant table -> f(Const<EXT>{}, Const<PLANT>{}): the run-time choice of the two template arguments the kernels share
template <class F>
auto with_ext_plant(bool ext, bool plant, F&& f) {
    if (plant) return ext ? f(Const<true>{}, Const<true>{}) : f(Const<false>{}, Const<true>{});
    return ext ? f(Const<true>{}, Const<false>{}) : f(Const<false>{}, Const<false>{});
}

// ------------------------------------------------------------------------------------------------
// small device helpers
// ------------------------------------------------------------------------------------------------
struct Mat3 {
    float r00, r01, r02, r10, r11, r12, r20, r21, r22;
    float m22;     // 1 - r22, computed directly (no cancellation for a near-level attitude)
};

__device__ __forceinline__ float fast_rcp(float x) { return __builtin_amdgcn_rcpf(x); }
__device__ __forceinline__ float fast_sqrt(float x) { return __builtin_amdgcn_sqrtf(x); }
__device__ __forceinline__ float fast_rsq(float x) { return __builtin_amdgcn_rsqf(x); }
// exp(x) for x <= 0 as 2^(x log2 e): v_exp_f32 (1 ulp) after one rounded product -- relative error <= (1 + |x|) 6e-8,
// two instructions instead of OCML's ~20.  Used for the downwash Gaussian (evaluated for every pair of an aviary).
__device__ __forceinline__ float fast_exp(float x) { return __builtin_amdgcn_exp2f(x * 1.44269504088896340736f); }

// Packed fp32 (v_pk_mul/add/fma_f32): TWO IEEE operations per instruction.  With one wave per SIMD the step is bound by
// the rate at which a single wave issues instructions (~5.4 cycles each, whatever they are -- scratch/issue.hip), not by
// the SIMD's arithmetic rate, so pairing two independent operations of the same kind halves their cost; each half
// rounds exactly like the scalar instruction, so results do not change by a bit.  Used only where both halves are
// naturally adjacent (no register shuffles); -fno-slp-vectorize keeps the compiler from pairing on its own (its
// shuffles cost more issue slots than the pairs save).
typedef float fp2 __attribute__((ext_vector_type(2)));
__device__ __forceinline__ fp2 fma2(fp2 a, fp2 b, fp2 c) { return __builtin_elementwise_fma(a, b, c); }
__device__ __forceinline__ fp2 splat(float s) { return fp2{s, s}; }

// Rare per-lane cases (gimbal lock, a tumbling drone, an episode end) are entered through a WAVE-UNIFORM test marked
// unlikely: the hot path pays one compare and one not-taken scalar branch (~11 cycles, scratch/issue.hip), and the
// rare block sits out of line.  The plain divergent `if` the compiler would emit instead -- s_and_saveexec +
// s_cbranch_execz around an in-line block -- costs a TAKEN branch (~60 cycles: the instruction buffer refills) on
// every step, and with one wave per SIMD nothing hides it.
__device__ __forceinline__ uint64_t lane_mask_opaque(bool p) {
    uint64_t m = __builtin_amdgcn_ballot_w64(p);
    asm volatile("" : "+s"(m));      // opaque: otherwise `if (any_lane(p)) if (p)` is folded back into the divergent `if (p)`
    return m;
}
// (a macro: __builtin_expect has to sit in the `if` itself -- returned from an inlined function it is dropped before inlining)
#define any_lane(p) __builtin_expect(lane_mask_opaque(p) != 0, 0)

// The three functions below are inlined at several places of the step kernel (rpy at the top of a step for
// DSLPID, at its tail for the observation, after an auto-reset).  FMA contraction is switched OFF inside them
// and every fused operation is written out, so that each inlined copy rounds identically: a K-step rollout
// carries the tail's rpy into the next step where a single-step launch recomputes it at the top, and the two
// must agree bit for bit.

// atan2 with the IEEE sign/quadrant conventions Bullet's Euler extraction relies on; minimax
// polynomial for atan(t)/t in t^2 on [0,1] (max abs error 7.4e-8 evaluated in fp32)
__device__ __forceinline__ float atan2_poly(float y, float x) {
#pragma clang fp contract(off)
    const float ax = fabsf(x), ay = fabsf(y);
    const float mx = fmaxf(ax, ay), mn = fminf(ax, ay);
    float t = mn * fast_rcp(mx);
    t = (mx == 0.0f) ? 0.0f : t;                 // atan2(0, 0) = 0
    const float u = t * t;
    float p = 2.766283504e-03f;
    p = fmaf(p, u, -1.573124913e-02f);
    p = fmaf(p, u, 4.213762361e-02f);
    p = fmaf(p, u, -7.456854827e-02f);
    p = fmaf(p, u, 1.061837064e-01f);
    p = fmaf(p, u, -1.419779779e-01f);
    p = fmaf(p, u, 1.999187203e-01f);
    p = fmaf(p, u, -3.333303671e-01f);
    p = fmaf(p, u, 9.999999818e-01f);
    p *= t;
    p = (ay > ax) ? (1.57079632679489661923f - p) : p;
    p = (x < 0.0f) ? (3.14159265358979323846f - p) : p;
    return copysignf(p, y);
}

// two independent atan2 at once: the same operations as atan2_poly, the multiplies and the Horner chain as packed pairs
__device__ __forceinline__ fp2 atan2_poly2(fp2 y, fp2 x) {
#pragma clang fp contract(off)
    const float ax0 = fabsf(x.x), ay0 = fabsf(y.x), ax1 = fabsf(x.y), ay1 = fabsf(y.y);
    const float mx0 = fmaxf(ax0, ay0), mn0 = fminf(ax0, ay0), mx1 = fmaxf(ax1, ay1), mn1 = fminf(ax1, ay1);
    fp2 t = fp2{mn0, mn1} * fp2{fast_rcp(mx0), fast_rcp(mx1)};
    t = fp2{(mx0 == 0.0f) ? 0.0f : t.x, (mx1 == 0.0f) ? 0.0f : t.y};   // atan2(0, 0) = 0
    const fp2 u = t * t;
    fp2 p = splat(2.766283504e-03f);
    p = fma2(p, u, splat(-1.573124913e-02f));
    p = fma2(p, u, splat(4.213762361e-02f));
    p = fma2(p, u, splat(-7.456854827e-02f));
    p = fma2(p, u, splat(1.061837064e-01f));
    p = fma2(p, u, splat(-1.419779779e-01f));
    p = fma2(p, u, splat(1.999187203e-01f));
    p = fma2(p, u, splat(-3.333303671e-01f));
    p = fma2(p, u, splat(9.999999818e-01f));
    p = p * t;
    float p0 = p.x, p1 = p.y;
    p0 = (ay0 > ax0) ? (1.57079632679489661923f - p0) : p0;
    p1 = (ay1 > ax1) ? (1.57079632679489661923f - p1) : p1;
    p0 = (x.x < 0.0f) ? (3.14159265358979323846f - p0) : p0;
    p1 = (x.y < 0.0f) ? (3.14159265358979323846f - p1) : p1;
    return fp2{copysignf(p0, y.x), copysignf(p1, y.y)};
}

// asin(s) = atan2(s, sqrt((1-s)(1+s))); the factored form keeps full relative accuracy near |s| = 1
__device__ __forceinline__ float asin_poly(float s) {
#pragma clang fp contract(off)
    return atan2_poly(s, fast_sqrt(fmaxf((1.0f - s) * (1.0f + s), 0.0f)));
}

// btMatrix3x3::setRotation (reached via p.getMatrixFromQuaternion, envs/BaseAviary.py:836);
// insensitive to |q| (DYN never renormalises q, SURVEY.md App. B.6)
__device__ __forceinline__ Mat3 quat_to_mat(float x, float y, float z, float w) {
    const float d = fmaf(x, x, fmaf(y, y, fmaf(z, z, w * w)));
    const float s = 2.0f * fast_rcp(d);
    const fp2 xys = fp2{x, y} * splat(s);                     // (packed pairs, see fma2)
    const float xs = xys.x, ys = xys.y, zs = z * s;
    const fp2 wxy = splat(w) * xys;
    const float wx = wxy.x, wy = wxy.y, wz = w * zs;
    Mat3 R;
    R.r00 = 1.0f - fmaf(y, ys, z * zs); R.r01 = fmaf(x, ys, -wz);           R.r02 = fmaf(x, zs, wy);
    R.r10 = fmaf(x, ys, wz);            R.r11 = 1.0f - fmaf(x, xs, z * zs); R.r12 = fmaf(y, zs, -wx);
    R.m22 = fmaf(x, xs, y * ys);
    R.r20 = fmaf(x, zs, -wy);           R.r21 = fmaf(y, zs, wx);            R.r22 = 1.0f - R.m22;
    return R;
}

// pybullet_getEulerFromQuaternion incl. its gimbal branches (envs/BaseAviary.py:518).  The regular branch is
// evaluated straight-line for every lane; the two gimbal branches (|sarg| >= 0.99999, i.e. pitch within 0.26 deg
// of +-90 deg) are a fix-up that is skipped unless some lane of the wave needs it.
__device__ __forceinline__ void quat_to_rpy(float x, float y, float z, float w,
                                            float& roll, float& pitch, float& yaw) {
#pragma clang fp contract(off)
    const float sarg = -2.0f * fmaf(x, z, -(w * y));
    const float ww_zz = fmaf(w, w, z * z);                       // squ + sqz
    const float xx_yy = fmaf(x, x, y * y);                       // sqx + sqy
    const float ww_yy = fmaf(w, w, -(y * y));                    // squ - sqy
    const float xx_zz = fmaf(x, x, -(z * z));                    // sqx - sqz
    // roll = atan2(2(yz + wx), squ - sqx - sqy + sqz), yaw = atan2(2(xy + wz), squ + sqx - sqy - sqz): evaluated together
    const fp2 ry = atan2_poly2(splat(2.0f) * fp2{fmaf(y, z, w * x), fmaf(x, y, w * z)}, fp2{ww_zz - xx_yy, ww_yy + xx_zz});
    roll = ry.x;
    pitch = asin_poly(fminf(fmaxf(sarg, -1.0f), 1.0f));          // (clamp: only matters on the gimbal lanes, overwritten below)
    yaw = ry.y;
    const bool gimbal = fabsf(sarg) >= 0.99999f;
    if (any_lane(gimbal)) {
        asm volatile("; gimbal lock: rare");                // (keeps the wave-uniform branch from being merged with the lane test)
        if (gimbal) {
            const bool neg = sarg < 0.0f;
            roll = 0.0f;
            pitch = neg ? -1.57079632679489661923f : 1.57079632679489661923f;
            yaw = 2.0f * (neg ? atan2_poly(x, -y) : atan2_poly(-x, y));
        }
    }
}

__device__ __forceinline__ float clampf(float v, float lo, float hi) {
    return fminf(fmaxf(v, lo), hi);   // np.clip
}

struct Kin {   // one drone's integrator state, all in VGPRs
    float px, py, pz, qx, qy, qz, qw, vx, vy, vz, wx, wy, wz;
};

struct Pid {   // DSLPIDControl members, control/DSLPIDControl.py:73-78
    float ipx, ipy, ipz, lr, lp, ly, irx, iry, irz;
};

// DSLPIDControl.computeControl (control/DSLPIDControl.py:82-145; SURVEY.md App. A.3).
// Returns the four RPMs; optionally the desired-vs-current yaw needed by the standalone entry.
__device__ __forceinline__ void dslpid(const GpdParams& P, float dt, float inv_dt, const Kin& k, float roll, float pitch,
                                       float yaw, const Mat3& R, float tx, float ty, float tz, float tyaw,
                                       float tvx, float tvy, float tvz, float trr, float trp, float try_,
                                       Pid& s, float rpm[4], float pos_e[3], float* yaw_e) {
    // ---- position loop, :187-203
    const float epx = tx - k.px, epy = ty - k.py, epz = tz - k.pz;
    const float evx = tvx - k.vx, evy = tvy - k.vy, evz = tvz - k.vz;
    s.ipx = clampf(fmaf(epx, dt, s.ipx), -2.0f, 2.0f);
    s.ipy = clampf(fmaf(epy, dt, s.ipy), -2.0f, 2.0f);
    s.ipz = clampf(clampf(fmaf(epz, dt, s.ipz), -2.0f, 2.0f), -0.15f, 0.15f);
    const float fx = fmaf(P.d_for[0], evx, fmaf(P.i_for[0], s.ipx, P.p_for[0] * epx));
    const float fy = fmaf(P.d_for[1], evy, fmaf(P.i_for[1], s.ipy, P.p_for[1] * epy));
    const float fz = fmaf(P.d_for[2], evz, fmaf(P.i_for[2], s.ipz, P.p_for[2] * epz)) + P.pid_gravity;
    const float along = fmaxf(0.0f, fmaf(fz, R.r22, fmaf(fy, R.r12, fx * R.r02)));
    const float base_pwm = (fast_sqrt(along * P.pid_inv_4kf) - P.pwm2rpm_const) * P.inv_pwm2rpm_scale;
    const float fn = fast_rsq(fmaf(fz, fz, fmaf(fy, fy, fx * fx)));
    const float zbx = fx * fn, zby = fy * fn, zbz = fz * fn;
    float sy, cy;
    sincosf(tyaw, &sy, &cy);                      // heading = [cos, sin, 0]
    float ybx = -(zbz * sy);                      // zb x heading
    float yby = zbz * cy;
    float ybz = fmaf(zbx, sy, -(zby * cy));
    const float yn = fast_rsq(fmaf(ybz, ybz, fmaf(yby, yby, ybx * ybx)));
    ybx *= yn; yby *= yn; ybz *= yn;
    const float xbx = fmaf(yby, zbz, -(ybz * zby));   // yb x zb
    const float xby = fmaf(ybz, zbx, -(ybx * zbz));
    const float xbz = fmaf(ybx, zby, -(yby * zbx));
    // ---- attitude loop, :240-259.  The reference rebuilds R* from its Euler angles through scipy;
    // that round trip returns the same orthonormal matrix (to 3e-16), so R* = [xb yb zb] is used.
    // e_R = vee(R*^T R - R^T R*): M_ij = col_i(R*) . col_j(R)
    const float m21 = fmaf(zbz, R.r21, fmaf(zby, R.r11, zbx * R.r01)), m12 = fmaf(ybz, R.r22, fmaf(yby, R.r12, ybx * R.r02));
    const float m02 = fmaf(xbz, R.r22, fmaf(xby, R.r12, xbx * R.r02)), m20 = fmaf(zbz, R.r20, fmaf(zby, R.r10, zbx * R.r00));
    const float m10 = fmaf(ybz, R.r20, fmaf(yby, R.r10, ybx * R.r00)), m01 = fmaf(xbz, R.r21, fmaf(xby, R.r11, xbx * R.r01));
    const float erx = m21 - m12, ery = m02 - m20, erz = m10 - m01;
    const float ewx = fmaf(-(roll - s.lr), inv_dt, trr);   // finite difference of Euler angles, no unwrap (:247)
    const float ewy = fmaf(-(pitch - s.lp), inv_dt, trp);
    const float ewz = fmaf(-(yaw - s.ly), inv_dt, try_);
    s.lr = roll; s.lp = pitch; s.ly = yaw;
    s.irx = clampf(clampf(fmaf(-erx, dt, s.irx), -1500.0f, 1500.0f), -1.0f, 1.0f);
    s.iry = clampf(clampf(fmaf(-ery, dt, s.iry), -1500.0f, 1500.0f), -1.0f, 1.0f);
    s.irz = clampf(fmaf(-erz, dt, s.irz), -1500.0f, 1500.0f);
    const float t0 = clampf(fmaf(P.i_tor[0], s.irx, fmaf(P.d_tor[0], ewx, -(P.p_tor[0] * erx))), -3200.0f, 3200.0f);
    const float t1 = clampf(fmaf(P.i_tor[1], s.iry, fmaf(P.d_tor[1], ewy, -(P.p_tor[1] * ery))), -3200.0f, 3200.0f);
    const float t2 = clampf(fmaf(P.i_tor[2], s.irz, fmaf(P.d_tor[2], ewz, -(P.p_tor[2] * erz))), -3200.0f, 3200.0f);
#pragma unroll
    for (int m = 0; m < 4; ++m) {
        const float pwm = clampf(fmaf(P.mixer[3 * m + 2], t2, fmaf(P.mixer[3 * m + 1], t1, fmaf(P.mixer[3 * m], t0, base_pwm))),
                                 P.min_pwm, P.max_pwm);
        rpm[m] = fmaf(P.pwm2rpm_scale, pwm, P.pwm2rpm_const);
    }
    if (pos_e) { pos_e[0] = epx; pos_e[1] = epy; pos_e[2] = epz; }
    if (yaw_e) {
        // yaw of the intrinsic-XYZ Euler angles of R* (scipy as_euler('XYZ'), :205): atan2(-R01, R00)
        *yaw_e = atan2_poly(-ybx, xbx) - yaw;
    }
}

// Thrust of one rotor as a deviation from the hover thrust F_h = GRAVITY/4 = KF*HOVER_RPM^2:
//   g = KF*rpm^2 - F_h = KF*(rpm - h)*(rpm + h) + (KF*h^2 - F_h),   h = float(HOVER_RPM)
// rpm - h is exact in fp32 (Sterbenz) for any rpm a quadrotor flies at, so g keeps ~1e-7 RELATIVE accuracy where
// KF*rpm^2 - F_h computed naively keeps 1e-7 of F_h -- 20..1000x coarser near hover.
__device__ __forceinline__ float thrust_dev(const GpdParams& P, float rpm) {
    return fmaf(P.KF * (rpm - P.hover_rpm), rpm + P.hover_rpm, P.hover_resid);
}
// ... and for the normalised action types, rpm = HOVER_RPM*(1 + e) (envs/BaseRLAviary.py:191-192):
//   g = F_h*((1 + e)^2 - 1) = F_h * e * (2 + e), with no reference to the rounded rpm at all
__device__ __forceinline__ float thrust_dev_norm(const GpdParams& P, float e) {
    return P.hover_thrust * (e * (2.0f + e));
}
__device__ __forceinline__ fp2 thrust_dev_norm2(const GpdParams& P, fp2 e) {     // (two rotors as a packed pair)
    return splat(P.hover_thrust) * (e * (splat(2.0f) + e));
}

// The plant path (gpd_rollout_plant, include/gpd.h GPD_PLANT_*): a lane-local copy of the nominal struct whose plant fields hold the
// lane's own drone (overwritten BY NAME from its row: the copy then lives in VGPRs, never in scratch).  `hover_thrust` is the drone's
// F_h = GRAVITY/4, the ground effect's KF*rpm^2 - g_i.  The normalised action types fly rpm = HOVER_RPM*(1 + e) of the NOMINAL airframe,
// whose thrust is T = s_kf * F_h,nominal (not the drone's F_h): their deviation is T*e*(2 + e) - (F_h - T).  The residual is SUBTRACTED:
// x - (+0) is x for every x, -0 included, so a nominal row (residual exactly 0) gives the uniform kernels' bits.
struct PlantParams : GpdParams {
    float norm_thrust;     // T = s_kf * F_h,nominal
    float norm_gap;        // F_h - T
};
__device__ __forceinline__ float thrust_dev_norm(const PlantParams& P, float e) {
    return P.norm_thrust * (e * (2.0f + e)) - P.norm_gap;
}
__device__ __forceinline__ fp2 thrust_dev_norm2(const PlantParams& P, fp2 e) {
    return splat(P.norm_thrust) * (e * (splat(2.0f) + e)) - splat(P.norm_gap);
}

// One physics sub-step (envs/BaseAviary.py:831-877 + :879-892), state in registers.
//   g[4]        rotor thrusts minus the hover thrust (KF*rpm_i^2 - GRAVITY/4), constant over the sub-steps
//   drag_rpm_sum  sum of the rpm the drag term sees (previous action on sub-step 0), only if DRAG
//   dw_force    body-z downwash force on this drone (already summed over the drones above), only if DW
// Forces are assembled from the deviations: total thrust T = GRAVITY + sum(g) (+ ground effect, downwash), so
//   F_z = R22*T - GRAVITY = R22*(T - GRAVITY) - GRAVITY*(1 - R22)      (1 - R22 computed directly)
// and the torques only see differences of the g_i (F_h cancels analytically: every torque row sums to zero).
//   AV          also produce the world angular velocity (only the LAST sub-step of an env step is observed)
template <bool EXT, bool AV = true>
__device__ __forceinline__ void substep(const GpdParams& P, float h, uint32_t flags, const float g[4],
                                        float drag_rpm_sum, float dw_force, Kin& k,
                                        float& avx, float& avy, float& avz) {
    const Mat3 R = quat_to_mat(k.qx, k.qy, k.qz, k.qw);
    float f0 = g[0], f1 = g[1], f2 = g[2], f3 = g[3];      // thrust deviations (ground effect adds to them)
    if (EXT && (flags & GPD_PHYS_GND)) {
        // per-rotor extra thrust (:739-743): KF*rpm_i^2 * coeff * (r/(4 h_i))^2, h_i = world z of rotor i, clipped
        // (the four rotors as two packed pairs: the same operations in the same order per rotor, half the issue slots)
        float e[4];
#pragma unroll
        for (int i = 0; i < 4; i += 2) {
            fp2 hz = fma2(splat(R.r21), fp2{P.prop_y[i], P.prop_y[i + 1]}, fma2(splat(R.r20), fp2{P.prop_x[i], P.prop_x[i + 1]}, splat(k.pz)));
            hz = fp2{fmaxf(hz.x, P.gnd_eff_h_clip), fmaxf(hz.y, P.gnd_eff_h_clip)};
            const fp2 ratio = splat(0.25f * P.prop_radius) * fp2{fast_rcp(hz.x), fast_rcp(hz.y)};
            const fp2 ei = ((splat(P.hover_thrust) + fp2{g[i], g[i + 1]}) * splat(P.gnd_eff_coeff)) * (ratio * ratio);
            e[i] = ei.x; e[i + 1] = ei.y;
        }
        // |roll| < pi/2 and |pitch| < pi/2 on Bullet's Euler extraction (:742), without the atan2/asin:
        // pitch = asin(sarg) is inside (-pi/2, pi/2) off the gimbal branches and exactly +-pi/2 on them;
        // roll = atan2(a, b) has |roll| < pi/2 iff b > 0 (or a == b == 0).  Same expressions as quat_to_rpy.
        const float sarg = -2.0f * fmaf(k.qx, k.qz, -(k.qw * k.qy));
        const float a = 2.0f * fmaf(k.qy, k.qz, k.qw * k.qx);
        const float b = fmaf(k.qw, k.qw, k.qz * k.qz) - fmaf(k.qx, k.qx, k.qy * k.qy);
        const bool on = (sarg > -0.99999f) && (sarg < 0.99999f) && (b > 0.0f || (a == 0.0f && b == 0.0f));
        if (on) { f0 += e[0]; f1 += e[1]; f2 += e[2]; f3 += e[3]; }
    }
    float dev = ((f0 + f1) + f2) + f3;                     // total thrust minus GRAVITY
    if (EXT && (flags & GPD_PHYS_DW)) dev += dw_force;
    const float T = P.GRAVITY + dev;
    const fp2 Fxy = fp2{R.r02, R.r12} * splat(T);
    float Fx = Fxy.x, Fy = Fxy.y, Fz = fmaf(R.r22, dev, -(P.GRAVITY * R.m22));
    if (EXT && (flags & GPD_PHYS_DRAG)) {
        // world force -DRAG_COEFF * v * sum(2*pi*rpm/60) (:771-774; R R^T cancels)
        const float wsum = drag_rpm_sum * (6.28318530717958647692f / 60.0f);
        Fx = fmaf(-(P.drag_coeff[0] * k.vx), wsum, Fx);
        Fy = fmaf(-(P.drag_coeff[1] * k.vy), wsum, Fy);
        Fz = fmaf(-(P.drag_coeff[2] * k.vz), wsum, Fz);
    }
    if (EXT && (flags & GPD_PHYS_DAMP)) {
        // Bullet's default multibody damping (NOT in the reference's Physics.DYN, see gpd.h): force -M d (1 + |v|) v
        const float vn = fast_sqrt(fmaf(k.vz, k.vz, fmaf(k.vy, k.vy, k.vx * k.vx)));
        const float ml = -(P.M * GPD_BULLET_DAMPING) * (1.0f + vn);
        Fx = fmaf(ml, k.vx, Fx); Fy = fmaf(ml, k.vy, Fy); Fz = fmaf(ml, k.vz, Fz);
    }
    // z torque from KM*rpm_i^2 = (KM/KF)*(F_h + g_i): alternating signs, F_h cancels (ground effect not included, :842).
    // The airframe variants are folded into signed constants and one bit-select: no branch and no per-step select chain
    // (negating a factor negates the product exactly, so the bits are those of "compute, then flip the sign").
    const float kz = (P.drone_model == GPD_MODEL_RACE) ? -P.km_over_kf : P.km_over_kf;
    const float tz = kz * (((-g[0] + g[1]) - g[2]) + g[3]);
    const float arm = P.L * 0.70710678118654752440f;        // L / sqrt(2)
    const float arm_x = (P.drone_model == GPD_MODEL_CF2X) ? -arm : arm;
    const float tx_x = (((f0 + f1) - f2) - f3) * arm_x, ty_x = (((-f0 + f1) + f2) - f3) * arm;   // CF2X / RACE
    const float tx_p = (f1 - f3) * P.L, ty_p = (-f0 + f2) * P.L;                                 // CF2P
    const uint32_t plus = (P.drone_model == GPD_MODEL_CF2P) ? 0xffffffffu : 0u;
    float tx = __uint_as_float((__float_as_uint(tx_p) & plus) | (__float_as_uint(tx_x) & ~plus));
    float ty = __uint_as_float((__float_as_uint(ty_p) & plus) | (__float_as_uint(ty_x) & ~plus));
    // Euler's rotation equation with diagonal J
    const fp2 jwxy = fp2{P.J[0], P.J[1]} * fp2{k.wx, k.wy};
    const float jwx = jwxy.x, jwy = jwxy.y, jwz = P.J[2] * k.wz;
    fp2 txy = fp2{tx, ty} - fp2{fmaf(k.wy, jwz, -(k.wz * jwy)), fmaf(k.wz, jwx, -(k.wx * jwz))};
    float tzz = tz - fmaf(k.wx, jwy, -(k.wy * jwx));
    if (EXT && (flags & GPD_PHYS_DAMP)) {                  // ... and torque -J w d (1 + |w|)
        const float wn = fast_sqrt(fmaf(k.wz, k.wz, fmaf(k.wy, k.wy, k.wx * k.wx)));
        const float da = -GPD_BULLET_DAMPING * (1.0f + wn);
        txy = fma2(jwxy, splat(da), txy);
        tzz = fmaf(jwz, da, tzz);
    }
    // semi-implicit Euler (:860-862): position uses the NEW velocity; x and y as packed pairs
    const fp2 hh = splat(h);
    const fp2 vxy = fma2(hh, fp2{Fx, Fy} * splat(P.inv_M), fp2{k.vx, k.vy});
    k.vx = vxy.x; k.vy = vxy.y; k.vz = fmaf(h, Fz * P.inv_M, k.vz);
    const fp2 wxy = fma2(hh, fp2{P.J_INV[0], P.J_INV[1]} * txy, fp2{k.wx, k.wy});
    k.wx = wxy.x; k.wy = wxy.y; k.wz = fmaf(h, P.J_INV[2] * tzz, k.wz);
    const fp2 pxy = fma2(hh, vxy, fp2{k.px, k.py});
    k.px = pxy.x; k.py = pxy.y; k.pz = fmaf(h, k.vz, k.pz);
    if (EXT && (flags & GPD_PHYS_GROUND)) {
        // the ground plane (NOT in the reference's Physics.DYN, see gpd.h): a drone whose collision cylinder would sink
        // below z = 0 is put back on the plane, loses its downward velocity (restitution 0) and sticks laterally
        // (second clause: a drone RESTING on the plane whose downward velocity is too small to move its fp32 height, h |vz| below
        // half an ulp of ground_z, would otherwise be neither caught nor free -- it slid laterally, unstuck, until vz had grown;
        // in exact arithmetic the clause only decides the tie pz == ground_z)
        const bool hit = (k.pz < P.ground_z) | ((k.pz <= P.ground_z) & (k.vz < 0.0f));
        k.pz = hit ? P.ground_z : k.pz;
        k.vz = hit ? fmaxf(k.vz, 0.0f) : k.vz;
        k.vx = hit ? 0.0f : k.vx;
        k.vy = hit ? 0.0f : k.vy;
    }
    // exact exponential quaternion update q <- q (x) exp(w h / 2)  (:879-892)
    //   q' = cos(t) q + (sin(t)/|w|) (q (x) [w,0]),  t = |w| h / 2.  cos(t) and sin(t)/t are even functions
    //   of t, evaluated as minimax polynomials in u = t^2 (abs err 7e-8 / 5e-8 for t <= 1 rad, i.e. body
    //   rates up to 480 rad/s at 240 Hz): no sqrt, no division, no range reduction.
    const float n2 = fmaf(k.wz, k.wz, fmaf(k.wy, k.wy, k.wx * k.wx));
    const float u = n2 * (0.25f * h * h);
    const fp2 uu = splat(u);                                  // (cos t, sin t / t): the two Horner chains as one packed chain
    const fp2 csp = fma2(fma2(fma2(fma2(fp2{2.412107309e-05f, 2.693749890e-06f}, uu, fp2{-1.388295778e-03f, -1.983586443e-04f}), uu,
                                  fp2{4.166645522e-02f, 8.333314057e-03f}), uu, fp2{-4.999999736e-01f, -1.666666643e-01f}), uu,
                        fp2{9.999999995e-01f, 1.0f});
    float cs = csp.x;
    float sc = csp.y * (0.5f * h);
    const bool tumbling = !(u <= 1.0f);                    // faster than 480 rad/s (at 240 Hz): exact path
    if (any_lane(tumbling)) {
        asm volatile("; tumbling: rare");
        if (tumbling) {
            const float n = sqrtf(n2);
            float sn;
            sincosf(n * h * 0.5f, &sn, &cs);
            sc = sn / n;
        }
    }
    {
        const float lx = fmaf(k.wx, k.qw, fmaf(k.wz, k.qy, -(k.wy * k.qz)));
        const float ly = fmaf(k.wy, k.qw, fmaf(k.wx, k.qz, -(k.wz * k.qx)));
        const float lz = fmaf(k.wz, k.qw, fmaf(k.wy, k.qx, -(k.wx * k.qy)));
        const float lw = -fmaf(k.wz, k.qz, fmaf(k.wy, k.qy, k.wx * k.qx));
        const bool turn = n2 > 1e-16f;                     // !np.isclose(|w|, 0): |w| <= 1e-8 keeps q  (select, no branch)
        const fp2 nxy = fma2(splat(sc), fp2{lx, ly}, splat(cs) * fp2{k.qx, k.qy});
        const fp2 nzw = fma2(splat(sc), fp2{lz, lw}, splat(cs) * fp2{k.qz, k.qw});
        k.qx = turn ? nxy.x : k.qx; k.qy = turn ? nxy.y : k.qy;
        k.qz = turn ? nzw.x : k.qz; k.qw = turn ? nzw.y : k.qw;
    }
    // world angular velocity handed to the state store: PRE-update rotation, post-update rates (:873)
    if (AV) {
        const fp2 axy = fma2(fp2{R.r02, R.r12}, splat(k.wz), fma2(fp2{R.r01, R.r11}, splat(k.wy), fp2{R.r00, R.r10} * splat(k.wx)));
        avx = axy.x; avy = axy.y;
        avz = fmaf(R.r22, k.wz, fmaf(R.r21, k.wy, R.r20 * k.wx));
    }
}

// SoA row access as  <uniform 64-bit row base in SGPRs> + <32-bit per-lane byte offset>: this is the
// global_load/store "saddr + voffset" form, one VGPR of address for all rows instead of a 64-bit
// add per access.  (gpd_step bounds N so that every byte offset fits 32 bits.)
__device__ __forceinline__ float ld_row(const float* __restrict__ base, int64_t ld, int r, uint32_t off4) {
    return *reinterpret_cast<const float*>(reinterpret_cast<const char*>(base + r * ld) + off4);
}
// The plant path: the lane's drone's row of the plant table ([GPD_PLANT_ROWS][ld], include/gpd.h) over a lane-local copy of the
// nominal struct -- the plant fields overwritten by name, everything else (the controller, the action mapping, the geometry) nominal.
// plant_of<false> is P itself: the uniform kernels' code does not change.
template <bool PLANT> using plant_t = std::conditional_t<PLANT, PlantParams, const GpdParams&>;
template <bool PLANT>
__device__ __forceinline__ plant_t<PLANT> plant_of(const GpdParams& P, const float* __restrict__ rows, int64_t ld, uint32_t off4) {
    if constexpr (PLANT) {
        PlantParams Q;
        static_cast<GpdParams&>(Q) = P;
        Q.M = ld_row(rows, ld, GPD_PLANT_M, off4);
        Q.inv_M = ld_row(rows, ld, GPD_PLANT_INV_M, off4);
        Q.KF = ld_row(rows, ld, GPD_PLANT_KF, off4);
        Q.GRAVITY = ld_row(rows, ld, GPD_PLANT_GRAVITY, off4);
        Q.J[0] = ld_row(rows, ld, GPD_PLANT_J, off4);
        Q.J[1] = ld_row(rows, ld, GPD_PLANT_J + 1, off4);
        Q.J[2] = ld_row(rows, ld, GPD_PLANT_J + 2, off4);
        Q.J_INV[0] = ld_row(rows, ld, GPD_PLANT_J_INV, off4);
        Q.J_INV[1] = ld_row(rows, ld, GPD_PLANT_J_INV + 1, off4);
        Q.J_INV[2] = ld_row(rows, ld, GPD_PLANT_J_INV + 2, off4);
        Q.km_over_kf = ld_row(rows, ld, GPD_PLANT_KM_OVER_KF, off4);
        Q.gnd_eff_coeff = ld_row(rows, ld, GPD_PLANT_GND_EFF, off4);
        Q.drag_coeff[0] = ld_row(rows, ld, GPD_PLANT_DRAG, off4);
        Q.drag_coeff[1] = ld_row(rows, ld, GPD_PLANT_DRAG + 1, off4);
        Q.drag_coeff[2] = ld_row(rows, ld, GPD_PLANT_DRAG + 2, off4);
        Q.hover_thrust = ld_row(rows, ld, GPD_PLANT_HOVER_THRUST, off4);
        Q.hover_resid = ld_row(rows, ld, GPD_PLANT_HOVER_RESID, off4);
        Q.norm_thrust = ld_row(rows, ld, GPD_PLANT_NORM_THRUST, off4);
        Q.norm_gap = ld_row(rows, ld, GPD_PLANT_NORM_GAP, off4);
        return Q;
    } else {
        (void)rows; (void)ld; (void)off4;
        return P;
    }
}
// the row's values live here (a kernel that claims its loads with an explicit wait names them before it)
template <bool PLANT>
__device__ __forceinline__ void plant_live(const plant_t<PLANT>& Q) {
    if constexpr (PLANT)
        asm volatile("" :: "v"(Q.M), "v"(Q.inv_M), "v"(Q.KF), "v"(Q.GRAVITY), "v"(Q.J[0]), "v"(Q.J[1]), "v"(Q.J[2]), "v"(Q.J_INV[0]),
                           "v"(Q.J_INV[1]), "v"(Q.J_INV[2]), "v"(Q.km_over_kf), "v"(Q.gnd_eff_coeff), "v"(Q.drag_coeff[0]),
                           "v"(Q.drag_coeff[1]), "v"(Q.drag_coeff[2]), "v"(Q.hover_thrust), "v"(Q.hover_resid), "v"(Q.norm_thrust),
                           "v"(Q.norm_gap) : "memory");
    else
        (void)Q;
}

template <bool NT = false>   // NT: non-temporal (a working set far beyond the caches is streamed, not kept)
__device__ __forceinline__ void st_row(float* __restrict__ base, int64_t ld, int r, uint32_t off4, float v) {
    float* p = reinterpret_cast<float*>(reinterpret_cast<char*>(base + r * ld) + off4);
    if (NT) __builtin_nontemporal_store(v, p);
    else *p = v;
}

// The kinematic block of GpdState (include/gpd.h, ABI 9): 13 x ld floats in four planes --
//   P  float4[ld] at kin          (pos x, pos y, pos z, body rate x)
//   Q  float4[ld] at kin + 4 ld   (quat x, y, z, w)
//   V  float4[ld] at kin + 8 ld   (vel x, vel y, vel z, body rate y)
//   W  float [ld] at kin + 12 ld  body rate z
// -- a lane moves its drone with three 16-byte and one 4-byte access per direction (rounds 1-4: thirteen rows of floats, 13 + 13
// accesses; the same bytes: -1 % per step at 65 536 drones, -5 % with DSLPID, -11 % at 4 194 304, profiles/r05_ab_step_kernel_round2.log).
__device__ __forceinline__ const float4* kin_P(const float* kin, int64_t ld) { (void)ld; return reinterpret_cast<const float4*>(kin); }
__device__ __forceinline__ const float4* kin_Q(const float* kin, int64_t ld) { return reinterpret_cast<const float4*>(kin + 4 * ld); }
__device__ __forceinline__ const float4* kin_V(const float* kin, int64_t ld) { return reinterpret_cast<const float4*>(kin + 8 * ld); }
__device__ __forceinline__ float4* kin_P(float* kin, int64_t ld) { (void)ld; return reinterpret_cast<float4*>(kin); }
__device__ __forceinline__ float4* kin_Q(float* kin, int64_t ld) { return reinterpret_cast<float4*>(kin + 4 * ld); }
__device__ __forceinline__ float4* kin_V(float* kin, int64_t ld) { return reinterpret_cast<float4*>(kin + 8 * ld); }

__device__ __forceinline__ void store_obs12(float* __restrict__ obs, uint32_t n, float px, float py, float pz,
                                            float roll, float pitch, float yaw, float vx, float vy, float vz,
                                            float ax, float ay, float az) {
    float4* o = reinterpret_cast<float4*>(reinterpret_cast<char*>(obs) + n * 48u);
    o[0] = make_float4(px, py, pz, roll);
    o[1] = make_float4(pitch, yaw, vx, vy);
    o[2] = make_float4(vz, ax, ay, az);
}

// ------------------------------------------------------------------------------------------------
// One env step of one drone, everything in registers.  Shared by the single-step kernel (gpd_step) and the
// rollout kernel (gpd_rollout): same statements in the same order, so K rollout steps are bitwise K single
// steps.
//   PID   : action types that run DSLPID (PID / VEL / ONE_D_PID)
//   EXT   : any of the GND/DRAG/DW terms may be enabled (flags tested at run time, uniformly)
//   MULTI : drones_per_env > 1 (env-level reductions and downwash go through LDS + workgroup barriers)
// ------------------------------------------------------------------------------------------------
// Workgroup barrier for LDS hand-offs: waits for this wave's outstanding LDS operations only (lgkmcnt), not for
// its global stores -- __syncthreads() would add a release fence, and with it a wait for every store in flight.
__device__ __forceinline__ void wg_barrier() {
    __builtin_amdgcn_s_waitcnt(0xC07F);                      // lgkmcnt(0); vmcnt / expcnt untouched
    __builtin_amdgcn_s_barrier();
}

struct Lane {             // which drone a lane works on
    uint32_t n;           // drone index (0 for a lane without a drone: it computes on drone 0 and stores nothing)
    uint32_t env;         // aviary index
    int tid;              // compute-lane index inside the workgroup (0 .. kBlock-1)
    int le, d;            // aviary / drone-in-aviary inside the workgroup
    int base;             // MULTI: the workgroup lane (tid) of the FIRST drone of this lane's aviary -- where the aviary's slots of the
                          // LDS exchange planes start
    bool active;
    bool shfl;            // MULTI: the D drones of an aviary are D consecutive lanes of ONE wave (D a power of two <= 64 in the
                          // single-step kernel; any D <= 64, whole aviaries per wave, in gpd_rollout1_kernel): they exchange through a
                          // wave-local LDS patch, without workgroup barriers
};

struct Carry {            // what a drone carries from one env step to the next
    Kin k;
    Pid s;                // DSLPID members
    float l0, l1, l2, l3; // last_clipped_action
    int counter;          // the aviary's step counter
    float dw_in;          // downwash force computed outside the kernel (one aviary of > 256 drones), else 0
    float roll, pitch, yaw;   // rpy of the cached pose (BaseAviary.py:518), carried from the tail of one step to
                              // the top of the next (DSLPID reads it there)
};

struct StepOut {          // what one env step hands to the stores
    float o[12];          // observation row: pos | rpy | vel | ang_v (of the reset pose if the aviary was reset)
    float to[12];         // last observation of the finished episode (meaningful only if `reset`)
    float rew;
    bool term, trunc, reset;
};

// action -> RPM (computed ONCE per env step from the cached state, BaseAviary.py:341) and the rotor thrusts minus the
// hover thrust.  DSLPID action types advance the controller members in c.s and read the cached rpy in c.
template <bool PID, int AW, int ACT, class PP>          // PP: GpdParams, or PlantParams (the plant path)
__device__ __forceinline__ void map_action(const PP& P, const GpdStepCfg& C, const float4 act, Carry& c,
                                           float rpm[4], float g[4]) {
    const Kin& k = c.k;
    const int act_type = ACT >= 0 ? ACT : C.act_type;
    rpm[0] = rpm[1] = rpm[2] = rpm[3] = 0.0f;
    if (!PID) {
        if (AW == 1) {     // GPD_ACT_ONE_D_RPM
            const float e = 0.05f * act.x;
            rpm[0] = rpm[1] = rpm[2] = rpm[3] = fmaf(P.hover_rpm, e, P.hover_rpm);
            g[0] = g[1] = g[2] = g[3] = thrust_dev_norm(P, e);
        } else if (act_type == GPD_ACT_RPM) {   // NOT clipped (SURVEY.md App. B.1)
            // rpm = HOVER_RPM*(1 + 0.05 a), g = thrust_dev_norm(0.05 a): rotors (0,1) and (2,3) as packed pairs
            const fp2 e01 = splat(0.05f) * fp2{act.x, act.y}, e23 = splat(0.05f) * fp2{act.z, act.w};
            const fp2 r01 = fma2(splat(P.hover_rpm), e01, splat(P.hover_rpm)), r23 = fma2(splat(P.hover_rpm), e23, splat(P.hover_rpm));
            const fp2 g01 = thrust_dev_norm2(P, e01), g23 = thrust_dev_norm2(P, e23);
            rpm[0] = r01.x; rpm[1] = r01.y; rpm[2] = r23.x; rpm[3] = r23.y;
            g[0] = g01.x; g[1] = g01.y; g[2] = g23.x; g[3] = g23.y;
        } else {           // GPD_ACT_RAW_RPM (clipped to [0, MAX_RPM], envs/CtrlAviary.py:140) or GPD_ACT_DIRECT_RPM (as is)
            const bool clip = act_type == GPD_ACT_RAW_RPM;
            const float lo = clip ? 0.0f : -3.0e38f, hi = clip ? P.max_rpm : 3.0e38f;
            rpm[0] = clampf(act.x, lo, hi); rpm[1] = clampf(act.y, lo, hi);
            rpm[2] = clampf(act.z, lo, hi); rpm[3] = clampf(act.w, lo, hi);
#pragma unroll
            for (int i = 0; i < 4; ++i) g[i] = thrust_dev(P, rpm[i]);
        }
    } else {
        float tx = k.px, ty = k.py, tz = k.pz, tyaw = 0.0f, tvx = 0.0f, tvy = 0.0f, tvz = 0.0f;
        if (AW == 3) {     // GPD_ACT_PID
            // waypoint limited to a 1 m approach step (_calculateNextStep, BaseAviary.py:1132-1150)
            const float dx = act.x - k.px, dy = act.y - k.py, dz = act.z - k.pz;
            const float d2 = fmaf(dz, dz, fmaf(dy, dy, dx * dx));
            if (fast_sqrt(d2) <= 1.0f) { tx = act.x; ty = act.y; tz = act.z; }
            else { const float id = fast_rsq(d2); tx = fmaf(dx, id, k.px); ty = fmaf(dy, id, k.py); tz = fmaf(dz, id, k.pz); }
        } else if (AW == 4) {   // GPD_ACT_VEL
            float ax = act.x, ay = act.y, az = act.z;
            float nn2 = fmaf(az, az, fmaf(ay, ay, ax * ax));
            // a tiny direction is a direction (include/gpd.h, GPD_ACT_VEL): below 2^-100 the squares are subnormal -- which the
            // reciprocal square root reads as zero -- or gone; 2^100 is exact and lifts the smallest subnormal's square to 2^-98
            if (nn2 < 0x1p-100f) { ax *= 0x1p100f; ay *= 0x1p100f; az *= 0x1p100f; nn2 = fmaf(az, az, fmaf(ay, ay, ax * ax)); }
            const float sp = P.speed_limit * fabsf(act.w);
            if (nn2 != 0.0f) { const float in = fast_rsq(nn2); tvx = sp * (ax * in); tvy = sp * (ay * in); tvz = sp * (az * in); }
            tyaw = c.yaw;                                 // keep the current yaw (:220)
        } else {   // GPD_ACT_ONE_D_PID
            tz = fmaf(0.1f, act.x, k.pz);
        }
        const Mat3 R = quat_to_mat(k.qx, k.qy, k.qz, k.qw);
        dslpid(P, C.ctrl_dt, C.inv_ctrl_dt, k, c.roll, c.pitch, c.yaw, R, tx, ty, tz, tyaw, tvx, tvy, tvz, 0.0f, 0.0f, 0.0f,
               c.s, rpm, nullptr, nullptr);
#pragma unroll
        for (int i = 0; i < 4; ++i) g[i] = thrust_dev(P, rpm[i]);
    }
}

// reward / terminated / truncated of a single-drone aviary (envs/HoverAviary.py:68-132); `counter` is the aviary's
// step counter BEFORE this step's increment (App. B.7)
__device__ __forceinline__ void task_single(const GpdStepCfg& C, float px, float py, float pz, float roll, float pitch,
                                            int counter, float tgx, float tgy, float tgz, float& rew, bool& term,
                                            bool& trunc) {
    const fp2 exy = fp2{tgx, tgy} - fp2{px, py};
    const float ex = exy.x, ey = exy.y, ez = tgz - pz;
    const float my_dist = fast_sqrt(fmaf(ez, ez, fmaf(ey, ey, ex * ex)));
    const float d2 = my_dist * my_dist;
    rew = fmaxf(0.0f, fmaf(-d2, d2, 2.0f));
    // (bitwise | on purpose: five compares and four scalar ORs instead of a short-circuit's exec-mask branches)
    const bool my_out = (fabsf(px) > C.xy_bound) | (fabsf(py) > C.xy_bound) | (pz > C.z_bound) |
                        (fabsf(roll) > C.tilt_bound) | (fabsf(pitch) > C.tilt_bound);
    term = my_dist < C.term_dist;
    trunc = my_out | (counter > C.trunc_counter);
}

// the value the neighbouring lane (lane ^ 1) holds: quad_perm [1, 0, 3, 2]
__device__ __forceinline__ float pair_mate(float v) {
    return __int_as_float(__builtin_amdgcn_mov_dpp(__float_as_int(v), 0xB1, 0xf, 0xf, true));
}

// ACT >= 0: the action type is a compile-time constant; S1: so is substeps == 1
template <bool PID, bool EXT, bool MULTI, int AW, int ACT = -1, bool S1 = false, class PP = GpdParams>
__device__ __forceinline__ void env_step(const PP& P, const GpdStepCfg& C, const uint32_t flags, const int D,
                                         const Lane& L, const float4 act, const float tgx, const float tgy,
                                         const float tgz, const bool ip_regs, const float* __restrict__ ipose,
                                         const float ip0, const float ip1, const float ip2, const float ip3,
                                         const float ip4, const float ip5, const float ip6, float* sh_pos,
                                         float* sh_red, Carry& c, StepOut& out, const float* irpy = nullptr) {
    Kin& k = c.k;
    float rpm[4], g[4];                                      // RPMs; rotor thrusts minus the hover thrust
    map_action<PID, AW, ACT>(P, C, act, c, rpm, g);

    // ---- S physics sub-steps, state in registers -------------------------------------------------
    const float cur_sum = ((rpm[0] + rpm[1]) + rpm[2]) + rpm[3];
    // the first sub-step of a step sees the PREVIOUS env step's action (BaseAviary.py:359,372)
    float drag_sum = (EXT && (flags & GPD_PHYS_DRAG)) ? ((c.l0 + c.l1) + c.l2) + c.l3 : cur_sum;
    float avx = 0.0f, avy = 0.0f, avz = 0.0f;
    if (S1 && !(EXT && MULTI)) {
        // ctrl_freq == pyb_freq, known at compile time: straight-line, no loop branches (two taken branches per step)
        substep<EXT>(P, C.pyb_dt, flags, g, drag_sum, EXT ? c.dw_in : 0.0f, k, avx, avy, avz);
    } else if (!MULTI) {
        // two sub-steps per iteration: half the loop branches (HoverAviary's default 30 Hz control is 8 sub-steps).  Only
        // the LAST sub-step's world angular velocity is observed (BaseAviary.py:873 overwrites it every sub-step), so the
        // loop covers all but the last one or two sub-steps without computing it.
        const float dw = EXT ? c.dw_in : 0.0f;
        int left = C.substeps;
        for (; left > 2; left -= 2) {
            substep<EXT, false>(P, C.pyb_dt, flags, g, drag_sum, dw, k, avx, avy, avz);
            substep<EXT, false>(P, C.pyb_dt, flags, g, cur_sum, dw, k, avx, avy, avz);
            drag_sum = cur_sum;
        }
        if (left == 2) {
            substep<EXT, false>(P, C.pyb_dt, flags, g, drag_sum, dw, k, avx, avy, avz);
            drag_sum = cur_sum;
        }
        substep<EXT, true>(P, C.pyb_dt, flags, g, drag_sum, dw, k, avx, avy, avz);
    } else
    for (int ss = 0, nsub = S1 ? 1 : C.substeps; ss < nsub; ++ss) {   // (S1 with MULTI: gpd_rollout1_kernel compiled for one aviary size)
        float dw = (EXT && !MULTI) ? c.dw_in : 0.0f;
        if (EXT && MULTI && (flags & GPD_PHYS_DW)) {
            // every drone sees the same pre-sub-step snapshot of its aviary (BaseAviary.py:346-347,798)
            auto wake_of = [&](float xj, float yj, float zj) {   // drone j above this one: its wake's push (:798-804)
                const float dz = zj - k.pz;
                const float ddx = xj - k.px, ddy = yj - k.py;
                const float dxy2 = fmaf(ddy, ddy, ddx * ddx);
                // evaluated for every mate and selected (no exec-mask branch per mate; a lane the test excludes may
                // compute inf/NaN here, which the select discards)
                const float ratio = (0.25f * P.prop_radius) * fast_rcp(dz);
                const float alpha = P.dw_coeff[0] * (ratio * ratio);
                const float beta = fmaf(P.dw_coeff[1], dz, P.dw_coeff[2]);
                const float ib = fast_rcp(beta);
                const float pushed = dw - alpha * fast_exp(-0.5f * (dxy2 * (ib * ib)));
                dw = ((dz > 0.0f) & (dxy2 < 100.0f)) ? pushed : dw;   // dz > 0 and dxy < 10 m
            };
            // Aviaries of more than two drones: the mates' coordinates cross LDS as three planes (x | y | z of the workgroup's lanes),
            // so that ONE read returns the same coordinate of consecutive mates as register pairs the packed instructions take as
            // they are (no moves), and the model runs for TWO mates per instruction wherever the operation exists in packed form
            // (differences, squares, the products around the two reciprocals and the exponential): ~15 issue slots per mate
            // instead of ~24.  Every operation is the scalar one (same rounding, same order) and a drone's sum still takes its
            // mates in index order: bit for bit what `wake_of` gives (scratch/exp_r06/ab_pairs.py holds digests against the
            // library before the change).
            // (the three coefficients as opaque scalars: splat(P.dw_coeff[i]) straight from the argument struct makes the compiler
            // read the array as overlapping 8-byte pairs from a COPY of it in scratch memory -- and a launch that needs scratch
            // costs ~0.3 us per step here, ab_pairs.py's first run)
            float dwc0 = P.dw_coeff[0], dwc1 = P.dw_coeff[1], dwc2 = P.dw_coeff[2];
            asm volatile("" : "+s"(dwc0), "+s"(dwc1), "+s"(dwc2));
            const fp2 mx = splat(k.px), my = splat(k.py), mz = splat(k.pz), qr = splat(0.25f * P.prop_radius);
            auto two_mates = [&](fp2 xj, fp2 yj, fp2 zj) {
                const fp2 dz = zj - mz, ddx = xj - mx, ddy = yj - my;
                const fp2 dxy2 = fma2(ddy, ddy, ddx * ddx);
                const fp2 ratio = qr * fp2{fast_rcp(dz.x), fast_rcp(dz.y)};
                const fp2 alpha = splat(dwc0) * (ratio * ratio);
                const fp2 beta = fma2(splat(dwc1), dz, splat(dwc2));
                const fp2 ib = fp2{fast_rcp(beta.x), fast_rcp(beta.y)};
                const fp2 arg = (splat(-0.5f) * (dxy2 * (ib * ib))) * splat(1.44269504088896340736f);   // fast_exp's product
                const fp2 push = alpha * fp2{__builtin_amdgcn_exp2f(arg.x), __builtin_amdgcn_exp2f(arg.y)};
                const float p0 = dw - push.x;
                dw = ((dz.x > 0.0f) & (dxy2.x < 100.0f)) ? p0 : dw;
                const float p1 = dw - push.y;
                dw = ((dz.y > 0.0f) & (dxy2.y < 100.0f)) ? p1 : dw;
            };
            const float* const sx = sh_pos + L.base;              // this aviary's x plane; y and z follow at kBlock, 2 kBlock
            auto pair_at = [&](int j) {                           // mates j, j + 1 (4-byte-aligned pairs: two dwords per LDS instruction)
                two_mates(fp2{sx[j], sx[j + 1]}, fp2{sx[kBlock + j], sx[kBlock + j + 1]}, fp2{sx[2 * kBlock + j], sx[2 * kBlock + j + 1]});
            };
            if (L.shfl) {
                // the aviary is D consecutive lanes of THIS wave: neither a workgroup barrier nor a wait between the writes and the
                // reads (the LDS executes a wave's instructions in order)
                if (D == 2) {
                    // a pair: the mate is the neighbouring lane -- three DPP moves (quad_perm [1,0,3,2]) instead of a trip through
                    // LDS, and the drone's own position (dz = 0: no contribution, whatever its turn in the reference's loop) is
                    // not evaluated at all
                    wake_of(pair_mate(k.px), pair_mate(k.py), pair_mate(k.pz));
                } else {
                    __builtin_amdgcn_wave_barrier();
                    sh_pos[L.tid] = k.px; sh_pos[kBlock + L.tid] = k.py; sh_pos[2 * kBlock + L.tid] = k.pz;
                    __builtin_amdgcn_wave_barrier();
                    if ((D & 3) == 0) {
                        // D = 4, 8 .. 64: groups of four mates, one 16-byte read per coordinate (the three reads of a group are issued
                        // together, and the loop branch -- a taken branch costs ~60 cycles at one wave per SIMD -- is paid once per group)
                        for (int j = 0; j < D; j += 4) {
                            const float4 x4 = *reinterpret_cast<const float4*>(sx + j);
                            const float4 y4 = *reinterpret_cast<const float4*>(sx + kBlock + j);
                            const float4 z4 = *reinterpret_cast<const float4*>(sx + 2 * kBlock + j);
                            two_mates(fp2{x4.x, x4.y}, fp2{y4.x, y4.y}, fp2{z4.x, z4.y});
                            two_mates(fp2{x4.z, x4.w}, fp2{y4.z, y4.w}, fp2{z4.z, z4.w});
                        }
                    } else {
                        // any other size that fits a wave (gpd_rollout1_kernel: whole aviaries per wave): 4-byte-aligned pairs
                        int j = 0;
                        for (; j + 4 <= D; j += 4) { pair_at(j); pair_at(j + 2); }
                        if (j + 2 <= D) { pair_at(j); j += 2; }
                        if (j < D) wake_of(sx[j], sx[kBlock + j], sx[2 * kBlock + j]);
                    }
                }
            } else {
                // any other size up to the workgroup's 256 lanes (the aviary may span waves: workgroup barriers; its first lane sits
                // at any multiple of D: 4-byte aligned pairs, which the LDS reads as two dwords in one instruction): four mates per
                // iteration, then the remaining 0 .. 3
                wg_barrier();
                sh_pos[L.tid] = k.px; sh_pos[kBlock + L.tid] = k.py; sh_pos[2 * kBlock + L.tid] = k.pz;
                wg_barrier();
                int j = 0;
                for (; j + 4 <= D; j += 4) { pair_at(j); pair_at(j + 2); }
                if (j + 2 <= D) { pair_at(j); j += 2; }
                if (j < D) wake_of(sx[j], sx[kBlock + j], sx[2 * kBlock + j]);
            }
        }
        substep<EXT>(P, C.pyb_dt, flags, g, drag_sum, dw, k, avx, avy, avz);
        drag_sum = cur_sum;
    }

    // ---- cache refresh: rpy of the new quaternion (BaseAviary.py:518) ------------------------------
    quat_to_rpy(k.qx, k.qy, k.qz, k.qw, c.roll, c.pitch, c.yaw);

    // ---- task: reward / terminated / truncated -------------------------------------------------------
    float rew = -1.0f;
    bool term = false, trunc = false;
    if (!MULTI) {
        // evaluated unconditionally and masked by the (uniform) task switch: selects, no branch in the step body
        // (GPD_TASK_NONE hands the kernel a readable dummy target)
        float r;
        bool te, tr;
        task_single(C, k.px, k.py, k.pz, c.roll, c.pitch, c.counter, tgx, tgy, tgz, r, te, tr);
        const bool has_task = C.task != GPD_TASK_NONE;
        rew = has_task ? r : -1.0f;
        term = has_task & te;
        trunc = has_task & tr;
    } else if (C.task != GPD_TASK_NONE) {
        {
            const float ex = tgx - k.px, ey = tgy - k.py, ez = tgz - k.pz;
            const float my_dist = fast_sqrt(fmaf(ez, ez, fmaf(ey, ey, ex * ex)));
            const float d2 = my_dist * my_dist;
            const float my_rew = fmaxf(0.0f, fmaf(-d2, d2, 2.0f));
            const bool my_out = fabsf(k.px) > C.xy_bound || fabsf(k.py) > C.xy_bound || k.pz > C.z_bound ||
                                fabsf(c.roll) > C.tilt_bound || fabsf(c.pitch) > C.tilt_bound;
            float r = 0.0f, dsum = 0.0f, o = 0.0f;
            const float my_o = my_out ? 1.0f : 0.0f;
            if (L.shfl && D == 2) {                            // a pair: the mate's three values by DPP (a + b either way round)
                r = my_rew + pair_mate(my_rew); dsum = my_dist + pair_mate(my_dist); o = my_o + pair_mate(my_o);
            } else if (L.shfl) {                               // wave-local LDS exchange, as for the downwash
                float4* sr = reinterpret_cast<float4*>(sh_red);
                __builtin_amdgcn_wave_barrier();
                sr[L.tid] = make_float4(my_rew, my_dist, my_o, 0.0f);
                __builtin_amdgcn_wave_barrier();
                const int base = L.base;
                auto mate = [&](int j) { const float4 v = sr[base + j]; r += v.x; dsum += v.y; o += v.z; };   // sequential, like the
                if ((D & 3) == 0) for (int j = 0; j < D; j += 4) { mate(j); mate(j + 1); mate(j + 2); mate(j + 3); }   // reference's loops
                else for (int j = 0; j < D; ++j) mate(j);
            } else {
                wg_barrier();
                sh_red[L.tid] = my_rew; sh_red[kBlock + L.tid] = my_dist; sh_red[2 * kBlock + L.tid] = my_o;
                wg_barrier();
                const int base = L.base;
                for (int j = 0; j < D; ++j) {                  // sequential, like the reference's loops
                    r += sh_red[base + j]; dsum += sh_red[kBlock + base + j]; o += sh_red[2 * kBlock + base + j];
                }
            }
            rew = r;
            term = dsum < C.term_dist;
            trunc = (o > 0.0f) || (c.counter > C.trunc_counter);
        }
    }
    const bool do_reset = C.auto_reset && (term || trunc);
    c.counter = do_reset ? 0 : c.counter + C.substeps;        // BaseAviary.py:382 / :460
    out.rew = rew; out.term = term; out.trunc = trunc; out.reset = do_reset;

    // ---- observation; same-step auto-reset ----------------------------------------------------------------
    c.l0 = rpm[0]; c.l1 = rpm[1]; c.l2 = rpm[2]; c.l3 = rpm[3];
    if (any_lane(do_reset)) { asm volatile("; episode end"); if (do_reset) {
        out.to[0] = k.px; out.to[1] = k.py; out.to[2] = k.pz; out.to[3] = c.roll; out.to[4] = c.pitch; out.to[5] = c.yaw;
        out.to[6] = k.vx; out.to[7] = k.vy; out.to[8] = k.vz; out.to[9] = avx; out.to[10] = avy; out.to[11] = avz;
        if (ip_regs) k = Kin{ip0, ip1, ip2, ip3, ip4, ip5, ip6, 0, 0, 0, 0, 0, 0};
        else k = Kin{ipose[0], ipose[1], ipose[2], ipose[3], ipose[4], ipose[5], ipose[6], 0, 0, 0, 0, 0, 0};
        // (the Euler angles of the reset pose: the K-step kernels compute them once per launch -- in the headline workload an
        // aviary of some wave's 64 ends its episode in one step out of six, and this block is what that wave then runs)
        if (irpy) { c.roll = irpy[0]; c.pitch = irpy[1]; c.yaw = irpy[2]; }
        else quat_to_rpy(k.qx, k.qy, k.qz, k.qw, c.roll, c.pitch, c.yaw);
        avx = avy = avz = 0.0f;
        c.l0 = c.l1 = c.l2 = c.l3 = 0.0f;                      // last_clipped_action zeroed (BaseAviary.py:468)
    } }
    out.o[0] = k.px; out.o[1] = k.py; out.o[2] = k.pz; out.o[3] = c.roll; out.o[4] = c.pitch; out.o[5] = c.yaw;
    out.o[6] = k.vx; out.o[7] = k.vy; out.o[8] = k.vz; out.o[9] = avx; out.o[10] = avy; out.o[11] = avz;
}

typedef float f4u __attribute__((ext_vector_type(4), aligned(4)));   // 16-byte vector at 4-byte alignment
typedef float f4v __attribute__((ext_vector_type(4)));

struct Span {             // internal: how the K steps of one launch are laid out in memory
    int32_t num_steps;
    int64_t action_stride;   // floats between the action blocks of consecutive steps (0: same action each step)
    int64_t obs_stride;      // floats between the obs12 (and term_obs12) blocks of consecutive steps
    int64_t env_stride;      // elements between the reward / terminated / truncated rows of consecutive steps
    int32_t ring;            // gpd_rollout: LDS output slots per workgroup (2 or 4), chosen at launch
};

// the raw action words of one drone (AW = 4, 3 or 1 floats per drone, row-major), one load instruction
template <int AW, bool NT = false>   // NT: read once, streamed in -- non-temporal
__device__ __forceinline__ float4 load_action(const float* __restrict__ action, uint32_t n) {
    const char* p = reinterpret_cast<const char*>(action) + n * static_cast<uint32_t>(AW * 4);
    if (AW == 1) {
        const float* ap = reinterpret_cast<const float*>(p);
        return make_float4(NT ? __builtin_nontemporal_load(ap) : *ap, 0.0f, 0.0f, 0.0f);
    }
    if (AW == 3) {
        const float* ap = reinterpret_cast<const float*>(p);
        if (NT) return make_float4(__builtin_nontemporal_load(ap), __builtin_nontemporal_load(ap + 1), __builtin_nontemporal_load(ap + 2), 0.0f);
        return make_float4(ap[0], ap[1], ap[2], 0.0f);
    }
    if (NT) {
        const f4v v = __builtin_nontemporal_load(reinterpret_cast<const f4v*>(p));
        return make_float4(v.x, v.y, v.z, v.w);
    }
    return *reinterpret_cast<const float4*>(p);
}

// Loads everything a launch needs once per drone: kinematics, DSLPID members, last RPMs, step counter, task
// target, (rollout: reset pose).  Branch-free on purpose: every load is issued back to back and ONE wait
// covers them all (a load inside a branch makes the compiler wait for it -- a full memory round trip --
// before the next one is even issued).  Lanes without a drone read drone 0's rows.
template <bool PID, bool EXT, bool IP = true>     // IP: also fetch the reset pose (rollouts; a single step reads it only when it resets)
__device__ __forceinline__ void load_carry(const GpdState& S, const GpdStepCfg& C, const uint32_t flags, const Lane& L,
                                           const float* __restrict__ target_pos, const float* __restrict__ ipl,
                                           Carry& c, float& tgx, float& tgy, float& tgz, float ip[7]) {
    const int64_t ld = S.ld;
    const uint32_t off4 = L.n * 4u;
    Kin& k = c.k;
    {   // the four planes of the kinematic block (include/gpd.h, GpdState.kin): three 16-byte loads and one 4-byte load per lane
        const uint32_t off16 = L.n * 16u;
        const f4v p = *reinterpret_cast<const f4v*>(reinterpret_cast<const char*>(S.kin) + off16);
        const f4v q = *reinterpret_cast<const f4v*>(reinterpret_cast<const char*>(S.kin + 4 * ld) + off16);
        const f4v v = *reinterpret_cast<const f4v*>(reinterpret_cast<const char*>(S.kin + 8 * ld) + off16);
        k.px = p.x; k.py = p.y; k.pz = p.z; k.wx = p.w;
        k.qx = q.x; k.qy = q.y; k.qz = q.z; k.qw = q.w;
        k.vx = v.x; k.vy = v.y; k.vz = v.z; k.wy = v.w;
        k.wz = ld_row(S.kin, ld, 12, off4);
    }
    c.counter = S.step_counter[L.env];                       // every drone of an aviary reads its aviary's counter
    GPD_DBG(c.counter >= 0, GPD_DBG_STEP_COUNTER, c.counter);
    // target (task NONE: the host passes a readable dummy, the values are not used)
    const float* tp = reinterpret_cast<const float*>(reinterpret_cast<const char*>(target_pos) +
                                                     (C.target_per_env ? L.n * 12u : static_cast<uint32_t>(L.d) * 12u));
    tgx = tp[0]; tgy = tp[1]; tgz = tp[2];
    c.s = Pid{0, 0, 0, 0, 0, 0, 0, 0, 0};
    if (PID) {
        Pid& s = c.s;
        s.ipx = ld_row(S.pid, ld, 0, off4); s.ipy = ld_row(S.pid, ld, 1, off4); s.ipz = ld_row(S.pid, ld, 2, off4);
        s.lr = ld_row(S.pid, ld, 3, off4); s.lp = ld_row(S.pid, ld, 4, off4); s.ly = ld_row(S.pid, ld, 5, off4);
        s.irx = ld_row(S.pid, ld, 6, off4); s.iry = ld_row(S.pid, ld, 7, off4); s.irz = ld_row(S.pid, ld, 8, off4);
    }
    c.l0 = c.l1 = c.l2 = c.l3 = 0.0f;
    c.dw_in = 0.0f;
    if (EXT) {
        // (the three pointers as VALUES before anything selects between them: `flag ? S.last_rpm : S.kin` on a GpdState that a kernel built
        // itself -- gpd_step_kernel, from its preloaded arguments -- otherwise becomes a load from a selected ADDRESS inside that struct, the
        // struct stays in scratch memory, and a launch that needs scratch costs 1.6 us more)
        const float* p_kin = S.kin;
        const float* p_rpm = S.last_rpm;
        const float* p_dw = S.dw_force;
        asm volatile("" : "+s"(p_kin), "+s"(p_rpm), "+s"(p_dw));
        // without the drag term the last RPMs are not needed: the loads then go to the (cached) first kin rows
        const float* lr = (flags & GPD_PHYS_DRAG) ? p_rpm : p_kin;
        c.l0 = ld_row(lr, ld, 0, off4); c.l1 = ld_row(lr, ld, 1, off4); c.l2 = ld_row(lr, ld, 2, off4); c.l3 = ld_row(lr, ld, 3, off4);
        const bool ext_dw = (flags & GPD_PHYS_DW) && p_dw != nullptr;
        const float v = ld_row(ext_dw ? p_dw : p_kin, ld, 0, off4);      // (unused case: a cached kin row)
        c.dw_in = ext_dw ? v : 0.0f;
    }
    if (IP) { ip[0] = ipl[0]; ip[1] = ipl[1]; ip[2] = ipl[2]; ip[3] = ipl[3]; ip[4] = ipl[4]; ip[5] = ipl[5]; ip[6] = ipl[6]; }
}

template <bool PID, bool NT = false>
__device__ __forceinline__ void store_carry(const GpdState& S, const Lane& L, const Carry& c) {
    const int64_t ld = S.ld;
    const uint32_t off4 = L.n * 4u;
    const Kin& k = c.k;
    if (L.d == 0) S.step_counter[L.env] = c.counter;
    if (S.bad) {
        // non-finite guard (include/gpd.h): a NaN or an infinity in any of the 13 floats makes the sum non-finite (inf - inf = NaN;
        // finite values of this magnitude cannot overflow it)
        const float sum = (((k.px + k.py) + (k.pz + k.qx)) + ((k.qy + k.qz) + (k.qw + k.vx))) + (((k.vy + k.vz) + (k.wx + k.wy)) + k.wz);
        // (the DSLPID members need no check: every one of them passes a clip or is overwritten each step -- control/
        // DSLPIDControl.py:191-193, 248-251 -- and v_max / v_min return the bound for a NaN where numpy's clip would propagate it.
        // For the same reason a NaN SET-POINT never reaches the state: one step of saturated commands, then the controller
        // recovers, where the reference's drone is gone for good.  tests/test_gpu_resume.py pins both behaviours.)
        S.bad[L.n] = fabsf(sum) <= 3.4028234e38f ? 0 : 1;
    }
    {
        const uint32_t off16 = L.n * 16u;
        // (opaque copies: without them the twelve field reads are combined into vector loads of the Carry struct, which then stays
        // an alloca -- promoted to LDS, indexed by a flat thread id computed from the DISPATCH PACKET, a read of host memory per wave:
        // 4.0 -> 14.6 us per step at 65 536 drones, profiles/r05_ab_step_kernel_round1.log)
        float e0 = k.px, e1 = k.py, e2 = k.pz, e3 = k.wx, e4 = k.qx, e5 = k.qy, e6 = k.qz, e7 = k.qw, e8 = k.vx, e9 = k.vy, e10 = k.vz, e11 = k.wy;
        asm volatile("" : "+v"(e0), "+v"(e1), "+v"(e2), "+v"(e3), "+v"(e4), "+v"(e5), "+v"(e6), "+v"(e7), "+v"(e8), "+v"(e9), "+v"(e10), "+v"(e11));
        const f4v p = {e0, e1, e2, e3}, q = {e4, e5, e6, e7}, v = {e8, e9, e10, e11};
        f4v* pp = reinterpret_cast<f4v*>(reinterpret_cast<char*>(S.kin) + off16);
        f4v* pq = reinterpret_cast<f4v*>(reinterpret_cast<char*>(S.kin + 4 * ld) + off16);
        f4v* pv = reinterpret_cast<f4v*>(reinterpret_cast<char*>(S.kin + 8 * ld) + off16);
        if (NT) { __builtin_nontemporal_store(p, pp); __builtin_nontemporal_store(q, pq); __builtin_nontemporal_store(v, pv); }
        else { *pp = p; *pq = q; *pv = v; }
        st_row<NT>(S.kin, ld, 12, off4, k.wz);
    }
    if (S.last_rpm) {
        st_row<NT>(S.last_rpm, ld, 0, off4, c.l0); st_row<NT>(S.last_rpm, ld, 1, off4, c.l1);
        st_row<NT>(S.last_rpm, ld, 2, off4, c.l2); st_row<NT>(S.last_rpm, ld, 3, off4, c.l3);
    }
    if (PID) {
        const Pid& s = c.s;
        st_row<NT>(S.pid, ld, 0, off4, s.ipx); st_row<NT>(S.pid, ld, 1, off4, s.ipy); st_row<NT>(S.pid, ld, 2, off4, s.ipz);
        st_row<NT>(S.pid, ld, 3, off4, s.lr); st_row<NT>(S.pid, ld, 4, off4, s.lp); st_row<NT>(S.pid, ld, 5, off4, s.ly);
        st_row<NT>(S.pid, ld, 6, off4, s.irx); st_row<NT>(S.pid, ld, 7, off4, s.iry); st_row<NT>(S.pid, ld, 8, off4, s.irz);
    }
}

// (BaseAviary._getDroneStateVector rows: shared by gpd_state_vectors and the one-world kernels)
// one row of BaseAviary._getDroneStateVector (envs/BaseAviary.py:541-561) from the SoA state and the obs12 row of the latest step
__device__ __forceinline__ void state20_row(const GpdState& S, const float* __restrict__ obs12, float* __restrict__ out, int64_t n) {
    const int64_t ld = S.ld;
    const float4 kp = kin_P(S.kin, ld)[n], kq = kin_Q(S.kin, ld)[n], kv = kin_V(S.kin, ld)[n];
    const float* o = obs12 + n * 12;
    float4* w = reinterpret_cast<float4*>(out + n * 20);
    const float l0 = S.last_rpm ? S.last_rpm[0 * ld + n] : 0.0f, l1 = S.last_rpm ? S.last_rpm[1 * ld + n] : 0.0f;
    const float l2 = S.last_rpm ? S.last_rpm[2 * ld + n] : 0.0f, l3 = S.last_rpm ? S.last_rpm[3 * ld + n] : 0.0f;
    w[0] = make_float4(kp.x, kp.y, kp.z, kq.x);
    w[1] = make_float4(kq.y, kq.z, kq.w, o[3]);
    w[2] = make_float4(o[4], o[5], kv.x, kv.y);
    w[3] = make_float4(kv.z, o[9], o[10], o[11]);
    w[4] = make_float4(l0, l1, l2, l3);
}

}  // namespace

