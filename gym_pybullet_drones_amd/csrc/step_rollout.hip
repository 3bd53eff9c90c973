// step_rollout.hip -- gpd_step / gpd_rollout / gpd_rollout_history: one env step per launch, K env steps per launch (DESIGN.md sections 3.1, 3.2)
#include "gpd_common.inc"
#include "policy_kernel.inc"
#include <iterator>
#include <utility>

namespace {

// ------------------------------------------------------------------------------------------------
// gpd_step: ONE env step per launch.  One lane per drone; the lane loads its state, steps, and stores state,
// observation row and the aviary's reward / flags itself (latency matters more than anything here: at
// N = 65 536 a launch lasts ~5 us).
// ------------------------------------------------------------------------------------------------
// ACT / S1: the action type and "one sub-step per step" as compile-time constants (no action-type ladder, no sub-step loop)
//
// The argument list STARTS with the fourteen dwords the load section needs (kernarg preload, `-mllvm -amdgpu-kernarg-preload-count=14`
// in _native.py: the command processor puts them into SGPRs before the wave starts, so the state / action / counter / target loads are
// issued without first waiting for a scalar load of the argument block -- one memory round trip off the launch's critical path; the
// by-value structs follow and are fetched while the vector loads are in flight).  Hot: copies of S.kin, S.step_counter, S.ld, the slot
// source (S.ring_pos, or the step counters when there is no ring), C.num_envs, C.lanes_per_wave, C.target_per_env.
// DC / FL: the aviary size and the physics flags as compile-time constants for BASELINE's multi-term shapes (0 / -1: from the argument
// block), as in gpd_rollout1_kernel below -- the uniform branches on them fold away, S1 then also applies to multi-drone aviaries.
// HI: with FL, whether the bits above the three add-on models (GPD_PHYS_GROUND, GPD_PHYS_DAMP: what a `Physics.PYB_*` member adds by default)
// are taken from the argument block (true) or known to be clear (false).
template <bool PID, bool EXT, bool MULTI, int AW, int ACT, bool S1, int DC = 0, int FL = -1, bool HI = false>
__global__ __launch_bounds__(kBlock) void gpd_step_kernel(
    float* __restrict__ hot_kin, const float* __restrict__ action, int32_t* __restrict__ hot_counter,
    const float* __restrict__ target_pos, const int32_t* __restrict__ hot_slot, const uint32_t hot_ld, const int32_t hot_num_envs,
    const int32_t hot_lanes_per_wave, const int32_t hot_target_per_env,
    const GpdParams P, const GpdState S_, const GpdStepCfg C_, const float* __restrict__ init_pose, float* __restrict__ obs12,
    float* __restrict__ reward, uint8_t* __restrict__ terminated, uint8_t* __restrict__ truncated,
    float* __restrict__ term_obs12, uint32_t* __restrict__ done_flag, const uint32_t done_seq) {
    constexpr bool PLANT = false;
    constexpr const float* plant = nullptr;
#include "step_kernel_body.inc"
}

// gpd_rollout_plant, one step: the generic entries of kStepVariants with a table of per-drone constants (the row is loaded with the state)
template <bool PID, bool EXT, bool MULTI, int AW, int ACT, bool S1>
__global__ __launch_bounds__(kBlock) void gpd_step_plant_kernel(
    float* __restrict__ hot_kin, const float* __restrict__ action, int32_t* __restrict__ hot_counter,
    const float* __restrict__ target_pos, const int32_t* __restrict__ hot_slot, const uint32_t hot_ld, const int32_t hot_num_envs,
    const int32_t hot_lanes_per_wave, const int32_t hot_target_per_env,
    const GpdParams P, const GpdState S_, const GpdStepCfg C_, const float* __restrict__ init_pose, float* __restrict__ obs12,
    float* __restrict__ reward, uint8_t* __restrict__ terminated, uint8_t* __restrict__ truncated,
    float* __restrict__ term_obs12, uint32_t* __restrict__ done_flag, const uint32_t done_seq, const float* __restrict__ plant) {
    constexpr int DC = 0, FL = -1;
    constexpr bool HI = false, PLANT = true;
#include "step_kernel_body.inc"
}

// ------------------------------------------------------------------------------------------------
// gpd_rollout: K env steps per launch.  The drone state is loaded ONCE, lives in VGPRs for all K steps and
// all sub-steps, and is stored ONCE.  A 320-thread workgroup holds two kinds of wavefronts:
//   * 4 COMPUTE waves (256 lanes, one drone each).  Per step a lane prefetches the NEXT step's action row from
//     HBM (its only global memory instruction in the loop, so the wait for it is a wait for loads only), steps,
//     and writes its observation row and the aviary's reward / flags to an LDS slot;
//   * 1 STORE wave that copies the previous step's LDS slot to HBM as fully coalesced 1 KiB dwordx4 bursts (the
//     row-major observation block of a workgroup is contiguous in memory, so the LDS hop also turns the compute
//     lanes' 48-byte-strided rows into whole cache lines).  It issues only stores and never waits for them.
// Why: gfx950 counts loads and stores on ONE in-order counter (vmcnt).  A wave that both prefetches its next
// action and stores its outputs can only wait for "the load" by also waiting for every store issued before
// it, and a store takes > 1 us to be acknowledged -- ~0.4 us per step measured at one wave per SIMD.  With the
// split, loads and stores live on different waves' counters and the only per-step synchronisation is one
// s_barrier (plus an LDS wait).
// ------------------------------------------------------------------------------------------------
constexpr int kStoreLanes = 64;
constexpr int kRollThreads = kBlock + kStoreLanes;
// LDS output ring (dynamic shared memory, sized at launch): `ring` slots of kSlotBytes each.  A small batch (one
// workgroup per CU) gets 4 slots -- the compute waves may run up to 3 steps ahead of the store wave; a large one
// gets 2 so that more workgroups fit a CU (160 KiB of LDS).  ring is a power of two.
constexpr int kSlotBytes = kBlock * 12 * 4 + kBlock * 4 + kBlock + kBlock;   // obs rows | rewards | terminated | truncated

// LDS flags of the compute-wave -> store-wave hand-off.  Plain volatile accesses are enough: one wave's LDS
// instructions execute in order, so a flag written after the data is seen after the data (the empty asm keeps the
// compiler from reordering them).
typedef __attribute__((address_space(3))) int lds_int_t;             // (explicit LDS address space: ds_read/ds_write, not flat)
typedef int i4v __attribute__((ext_vector_type(4)));
typedef __attribute__((address_space(3))) i4v lds_i4v_t;
__device__ __forceinline__ int lds_peek(int* p) { return *reinterpret_cast<volatile lds_int_t*>((lds_int_t*)p); }
__device__ __forceinline__ i4v lds_peek4(int* p) { return *reinterpret_cast<volatile lds_i4v_t*>((lds_i4v_t*)p); }
__device__ __forceinline__ void lds_poke(int* p, int v) {
    asm volatile("" ::: "memory");
    *reinterpret_cast<volatile lds_int_t*>((lds_int_t*)p) = v;
    asm volatile("" ::: "memory");
}



// ACT / S1: the action type and "one sub-step per step" as compile-time constants, as in the other two kernels (ACT = -1: the run-time
// ladder, which multi-drone aviaries keep -- their steps are dominated by the exchange and the barriers)
template <bool PID, bool EXT, bool MULTI, int AW, int ACT = -1, bool S1 = false>
__global__ __launch_bounds__(kRollThreads) void gpd_rollout_kernel(
    const GpdParams P, const GpdState S, const GpdStepCfg C, const Span T, const float* __restrict__ action,
    const float* __restrict__ target_pos, const float* __restrict__ init_pose, float* __restrict__ obs12,
    float* __restrict__ reward, uint8_t* __restrict__ terminated, uint8_t* __restrict__ truncated,
    float* __restrict__ term_obs12) {
    constexpr bool PLANT = false;
    constexpr const float* plant = nullptr;
#include "rollout_kernel_body.inc"
}

// gpd_rollout_plant with terminal observations or aviaries of more than 64 drones: gpd_rollout_kernel with the plant table
template <bool PID, bool EXT, bool MULTI, int AW, int ACT, bool S1>
__global__ __launch_bounds__(kRollThreads) void gpd_rollout_plant_kernel(
    const GpdParams P, const GpdState S, const GpdStepCfg C, const Span T, const float* __restrict__ action,
    const float* __restrict__ target_pos, const float* __restrict__ init_pose, float* __restrict__ obs12,
    float* __restrict__ reward, uint8_t* __restrict__ terminated, uint8_t* __restrict__ truncated,
    float* __restrict__ term_obs12, const float* __restrict__ plant) {
    constexpr bool PLANT = true;
#include "rollout_kernel_body.inc"
}

// ------------------------------------------------------------------------------------------------
// Per-step outputs of a single-drone rollout lane (shared by the two kernels below).
//   * observation row -> the wave's LDS patch -> three coalesced 1 KiB bursts (the 64 rows of a wave are contiguous in
//     memory), software-pipelined by one step: the bursts of step t - 1, read back from the patch a whole step ago (the
//     LDS round trip is never waited for), go out first; then this step's row is written to the patch and read back
//     into `pend`.  Same wave on both sides: the LDS executes a wave's instructions in order, so the reads see the
//     writes without any wait or barrier (the wave_barrier only pins the order for the compiler).  At step 0 the bursts
//     carry zeros to step 0's rows, which step 1 then overwrites (same lane, same addresses, program order): every
//     store is unconditional.
//   * reward and flags go out directly (already coalesced).
//   * addressing: <uniform running pointer in SGPRs> + <32-bit lane offset>, the global_store "saddr + voffset" form;
//     the empty asm keeps the zero-extension of the offsets inside the loop (hoisted, it turns every store into a
//     64-bit VALU add plus a flat-addressed store).
// ------------------------------------------------------------------------------------------------
template <bool NT_OBS = true>     // NT_OBS: the observation bursts are stored non-temporally (see launch_step for when not)
struct RollOut {
    char* og_prev; char* og; char* rg; uint8_t* tg; uint8_t* ug;     // obs block of the previous / this step, reward, flags
    int64_t obs_step, env_step;                                     // bytes / elements between consecutive steps
    uint32_t g0, g1, g2, e4, e1;                                    // lane offsets: three bursts, reward word, flag byte
    float4* mine; const char* lsrc;                                 // this lane's row in the patch; its three burst chunks
    f4v pend[3];                                                    // the previous step's three bursts
    __device__ __forceinline__ RollOut(float* obs12, float* reward, uint8_t* terminated, uint8_t* truncated, const Span& T,
                                       const uint32_t goff[3], uint32_t eoff4, uint32_t env, float* row, const char* lsrc_)
        : og_prev(reinterpret_cast<char*>(obs12)), og(reinterpret_cast<char*>(obs12)), rg(reinterpret_cast<char*>(reward)),
          tg(terminated), ug(truncated), obs_step(T.obs_stride * 4), env_step(T.env_stride), g0(goff[0]), g1(goff[1]),
          g2(goff[2]), e4(eoff4), e1(env), mine(reinterpret_cast<float4*>(row)), lsrc(lsrc_) {
        pend[0] = pend[1] = pend[2] = f4v{0, 0, 0, 0};
    }
    __device__ __forceinline__ void bursts(char* base) {
        asm volatile("" : "+v"(g0), "+v"(g1), "+v"(g2));
        if (NT_OBS) {
            __builtin_nontemporal_store(pend[0], reinterpret_cast<f4v*>(base + g0));   // written once, streamed out
            __builtin_nontemporal_store(pend[1], reinterpret_cast<f4v*>(base + g1));
            __builtin_nontemporal_store(pend[2], reinterpret_cast<f4v*>(base + g2));
        } else {
            *reinterpret_cast<f4v*>(base + g0) = pend[0];
            *reinterpret_cast<f4v*>(base + g1) = pend[1];
            *reinterpret_cast<f4v*>(base + g2) = pend[2];
        }
    }
    // `advance`: false on the first step of the launch (the pointers already address step 0)
    __device__ __forceinline__ void emit(const StepOut& out, bool advance) {
        if (advance) { og_prev = og; og += obs_step; rg += env_step * 4; tg += env_step; ug += env_step; }
        bursts(og_prev);
        mine[0] = make_float4(out.o[0], out.o[1], out.o[2], out.o[3]);
        mine[1] = make_float4(out.o[4], out.o[5], out.o[6], out.o[7]);
        mine[2] = make_float4(out.o[8], out.o[9], out.o[10], out.o[11]);
        __builtin_amdgcn_wave_barrier();
#pragma unroll
        for (int j = 0; j < 3; ++j) {
            const float4 v = *reinterpret_cast<const float4*>(lsrc + j * 1024);
            pend[j] = f4v{v.x, v.y, v.z, v.w};
        }
        __builtin_amdgcn_wave_barrier();                             // (the next step's row writes stay behind these reads)
        asm volatile("" : "+v"(e4), "+v"(e1));
        __builtin_nontemporal_store(out.rew, reinterpret_cast<float*>(rg + e4));
        __builtin_nontemporal_store(static_cast<uint8_t>(out.term ? 1 : 0), tg + e1);
        __builtin_nontemporal_store(static_cast<uint8_t>(out.trunc ? 1 : 0), ug + e1);
    }
    __device__ __forceinline__ void flush() { bursts(og); }          // after the last step
};

// ------------------------------------------------------------------------------------------------
// gpd_rollout for single-drone aviaries: K env steps per launch with NO helper wave and NO workgroup
// synchronisation at all.  256-thread workgroups, one drone per lane; per step a lane
//   * prefetches the action row two steps ahead (three rotating register sets, loop unrolled x3),
//   * steps (env_step, everything in registers),
//   * writes its 48-byte observation row into its wave's 3 KiB LDS patch, and the wave stores the patch as three
//     fully coalesced 1 KiB dwordx4 bursts (the 64 rows of a wave are contiguous in memory); reward and flags go
//     out directly (already coalesced).
// Every global memory instruction of the loop body is UNCONDITIONAL -- this is what makes it fast: gfx950 counts
// loads and stores on one in-order counter, and only with a fixed number of operations per step can the wait for
// "the row requested two steps ago" be an exact `vmcnt(14)` (the two younger loads and the twelve stores of the two
// steps in between may still be in flight) instead of a wait for every store issued so far (a store takes > 1 us
// to be acknowledged).  Lanes without a drone (ragged last workgroup) are exact CLONES of the first drone of their
// own workgroup -- same state, same action row, same arithmetic, hence the same bits -- and store to that drone's
// addresses: a benign duplicate write instead of a branch around the stores.  (Calls that ask for terminal observations -- conditional stores -- use
// the compute-wave + store-wave kernel above.)
// ------------------------------------------------------------------------------------------------
// MULTI: aviaries of D = 2 .. 64 drones, WHOLE aviaries per wave ((64 / D) D lanes of a wave hold a drone: D consecutive lanes of one
// wave per aviary, wave-local exchange inside env_step, no workgroup barrier).  Every lane of an aviary ends a step with the
// aviary's reward and flags and stores them to the aviary's slot -- D identical writes instead of a branch; a lane without a drone
// is a clone (the lane mapping in the kernel says of whom), so clones replay their originals bit for bit.
// RING (gpd_rollout_history): every step's raw action is also pushed into the action ring, like gpd_step does (slots q and
// q + H of the double ring; two more stores per lane and step, which the explicit wait counts of the loop include because
// they are unconditional -- a compile-time variant, not a run-time test).
// (the argument list starts with the fourteen dwords the launch's first loads need -- kernarg preload, as for gpd_step_kernel: the state,
// the first action rows, the counter, the target and the reset pose are requested without first waiting for the argument block)
// DC: the aviary size as a compile-time constant (0: C.drones_per_env) -- BASELINE's two multi-drone shapes, pairs (config 5) and stacks of
// eight (config 3 ii), at one sub-step per step: the size tests, the mates loops of the downwash and of the task sums and the sub-step loop
// fold away, the LDS reads of all mates are issued together and no loop branch is taken (a taken branch costs ~60 cycles at one wave per
// SIMD).  Same operations in the same order: bit for bit the generic kernel (scratch/exp_r06/ab_unroll.py).
// FL: the physics flags as a compile-time constant too (-1: C.physics_flags) -- the reference's two multi-drone add-on sets, PYB_DW (4) and
// PYB_GND_DRAG_DW (7): the flag tests of every sub-step (uniform branches: ~11 cycles not taken, 25-60 taken) fold away.
// HI: with FL, the bits above the add-on models (the ground plane and Bullet's damping, which `Physics.PYB_*` members add by default) come
// from the argument block (true) or are known to be clear (false: exactly the reference's explicit integrator + the add-on models).
template <bool PID, bool EXT, int AW, int ACT, bool S1, bool MULTI, bool NT_OBS = true, bool RING = false, int DC = 0, int FL = -1, bool HI = false>
__global__ __launch_bounds__(kBlock) void gpd_rollout1_kernel(
    float* __restrict__ hot_kin, const float* __restrict__ action, int32_t* __restrict__ hot_counter, const float* __restrict__ target_pos,
    const float* __restrict__ init_pose, const uint32_t hot_ld, const int32_t hot_num_envs, const int32_t hot_num_steps, const uint32_t hot_bits,
    const GpdParams P, const GpdState S_, const GpdStepCfg C_, const Span T_, float* __restrict__ obs12,
    float* __restrict__ reward, uint8_t* __restrict__ terminated, uint8_t* __restrict__ truncated,
    float* __restrict__ term_obs12) {
    constexpr bool PLANT = false;
    constexpr const float* plant = nullptr;
#include "rollout1_kernel_body.inc"
}

// gpd_rollout_plant, K > 1 steps without terminal observations, aviaries of up to 64 drones: the generic entries of kRoll1Variants with
// the plant table (non-temporal observation bursts, no action ring), the row loaded with the state and kept in registers for the K steps
template <bool PID, bool EXT, int AW, int ACT, bool S1, bool MULTI>
__global__ __launch_bounds__(kBlock) void gpd_rollout1_plant_kernel(
    float* __restrict__ hot_kin, const float* __restrict__ action, int32_t* __restrict__ hot_counter, const float* __restrict__ target_pos,
    const float* __restrict__ init_pose, const uint32_t hot_ld, const int32_t hot_num_envs, const int32_t hot_num_steps, const uint32_t hot_bits,
    const GpdParams P, const GpdState S_, const GpdStepCfg C_, const Span T_, float* __restrict__ obs12,
    float* __restrict__ reward, uint8_t* __restrict__ terminated, uint8_t* __restrict__ truncated,
    float* __restrict__ term_obs12, const float* __restrict__ plant) {
    constexpr bool NT_OBS = true, RING = false, HI = false, PLANT = true;
    constexpr int DC = 0, FL = -1;
#include "rollout1_kernel_body.inc"
}

// ------------------------------------------------------------------------------------------------
// Which compiled kernel serves a call.  gpd_step_kernel and gpd_rollout1_kernel each have ONE ordered list of compile-time variants,
// and the first entry that fits the call wins.  An entry holds the kernels' template parameters MULTI, S1, DC, FL, HI:
//   multi  whole aviaries, or single drones;
//   s1     one sub-step per step (false: the sub-step loop);
//   dc     the aviary size (0: from the argument block);
//   fl     the three add-on models, GPD_PHYS_GND | GPD_PHYS_DRAG | GPD_PHYS_DW (-1: every flag from the argument block);
//   hi     with fl: the bits above them -- the ground plane and Bullet's damping, which `Physics.PYB_*` members add by default -- come
//          from the argument block (true) or are known to be clear (false: exactly the reference's explicit integrator + add-ons).
// A SIZED entry fixes the size or the flags, or one sub-step for whole aviaries: the uniform branches on them fold away (DESIGN.md
// section 3.2; the gains below are per env step at 65 536 drones, 64 steps per launch).  Sized entries are compiled for BaseRLAviary's
// five action types only (not for the raw-RPM rows of CtrlAviary and of subclasses with their own _preprocessAction: every variant is
// another pair of large kernels to compile), those with a flag set only where flags are set (EXT).  Each list ends with the generic
// entries, which fit every call of their shape.
// GPD_ROLLOUT_SIZED=0 is a TEST HOOK, read once per process: no sized entry fits, the generic kernels serve every call -- they are the
// reference of tests/test_gpu_rollout.py's bit-for-bit comparison of the sized kernels inside the shipped library.
// ------------------------------------------------------------------------------------------------
template <int ACT> constexpr bool kSizedAct = ACT != GPD_ACT_RAW_RPM && ACT != GPD_ACT_DIRECT_RPM;

struct Variant {
    bool multi, s1;
    int dc, fl;
    bool hi;
    constexpr bool sized() const { return dc != 0 || fl >= 0 || (multi && s1); }
    bool fits(const GpdStepCfg& C) const {
        return multi == (C.drones_per_env > 1) && (!s1 || C.substeps == 1) && (dc == 0 || dc == C.drones_per_env) &&
               (fl < 0 || ((C.physics_flags & 7u) == static_cast<uint32_t>(fl) && (hi || (C.physics_flags & ~7u) == 0u)));
    }
};
template <bool EXT, int ACT> constexpr bool compiled(const Variant& v) { return !v.sized() || (kSizedAct<ACT> && (EXT || v.fl < 0)); }

// gpd_step_kernel: one env step per launch (its one-wave launches ARE the drop-in aviaries' step())
constexpr Variant kStepVariants[] = {
    // BASELINE configs 3 (ii), 5 and 3 (i) at one sub-step per step, upper bits clear or read (as in gpd_rollout1_kernel)
    {true, true, 8, 7, false}, {true, true, 8, 7, true}, {true, true, 2, 4, false}, {true, true, 2, 4, true},
    {false, true, 0, 7, false}, {false, true, 0, 7, true},
    // the two multi-drone add-on sets under the sub-step loop (30 Hz control of 240 Hz physics is the reference's default), upper bits
    // read (single drones would gain 3-5 % there: no variant)
    {true, false, 8, 7, true}, {true, false, 2, 4, true},
    // no add-on model, the ground plane / damping bits alone -- what `Physics.PYB`, the default of HoverAviary() and MultiHoverAviary(),
    // resolves to -- for single drones and pairs, one sub-step or the loop: HoverAviary().step() 22.1-23.9 -> 18.9-19.4 us
    {false, true, 0, 0, true}, {false, false, 0, 0, true}, {true, true, 2, 0, true}, {true, false, 2, 0, true},
    // generic
    {true, false, 0, -1, false}, {false, true, 0, -1, false}, {false, false, 0, -1, false},
};

// gpd_rollout1_kernel: K env steps per launch, whole aviaries of up to 64 drones per wave or single drones
constexpr Variant kRoll1Variants[] = {
    // pairs with PYB_DW, stacks of eight with PYB_GND_DRAG_DW (BASELINE configs 5 and 3 ii), any size with every add-on, at one sub-step,
    // upper bits clear or read: pairs 1.087 -> 0.777 us, stacks 1.827 -> 1.356, other sizes -10 .. -15 %, with the upper bits -16 .. -18 %
    {true, true, 8, 7, false}, {true, true, 8, 7, true}, {true, true, 2, 4, false}, {true, true, 2, 4, true},
    {true, true, 0, 7, false}, {true, true, 0, 7, true},
    // the same under the sub-step loop (30 Hz control), upper bits read: pairs -24 %, stacks -18 %, other sizes -7 %
    {true, false, 8, 7, true}, {true, false, 2, 4, true}, {true, false, 0, 7, true},
    // pairs with no add-on model and the ground plane / damping bits alone: MultiHoverAviary's defaults (`Physics.PYB`, 30 Hz: -21 %)
    {true, true, 2, 0, true}, {true, false, 2, 0, true},
    // pairs with any other flags (-7 % without add-on forces), any size, at one sub-step (0 .. -6 %; under the loop the size buys nothing)
    {true, true, 2, -1, false}, {true, true, 0, -1, false},
    // single drones with every add-on model (BASELINE config 3 i: 1.053 -> 0.927 us, upper bits read -5 %), or with none and the ground
    // plane / damping bits alone (`Physics.PYB`: -9 % at 240 Hz, -18.5 % at 30 Hz)
    {false, true, 0, 7, false}, {false, true, 0, 7, true}, {false, true, 0, 0, true}, {false, false, 0, 0, true},
    // generic (also gpd_rollout_history's, with the action ring, and the headline's: launch_step)
    {true, false, 0, -1, false}, {false, true, 0, -1, false}, {false, false, 0, -1, false},
};

inline bool sized_variants() {
    static const bool on = [] { const char* e = getenv("GPD_ROLLOUT_SIZED"); return e == nullptr || e[0] != '0'; }();
    return on;
}

template <auto V> using Const = std::integral_constant<decltype(V), V>;

// f(Const<i>{}) -- instantiated for the entries of LIST this <EXT, ACT> compiles, and only for them
template <const auto& LIST, bool EXT, int ACT, class F, size_t... I>
void launch_entry(size_t i, F& f, std::index_sequence<I...>) {
    auto at = [&](auto J) { if constexpr (compiled<EXT, ACT>(LIST[decltype(J)::value])) f(J); };
    ((i == I ? at(Const<I>{}) : void()), ...);
}

// the first entry of LIST that is compiled and fits the call (sized entries only while `sized`)
template <const auto& LIST, bool EXT, int ACT, class F>
hipError_t launch_first_fit(bool sized, const GpdStepCfg& C, F&& f) {
    for (size_t i = 0; i < std::size(LIST); ++i)
        if (compiled<EXT, ACT>(LIST[i]) && (sized || !LIST[i].sized()) && LIST[i].fits(C)) {
            launch_entry<LIST, EXT, ACT>(i, f, std::make_index_sequence<std::size(LIST)>{});
            return hipGetLastError();
        }
    return hipErrorInvalidDeviceFunction;                    // (not reached: a generic entry fits every call)
}

// PLANT (gpd_rollout_plant): the three plant kernels, built from the GENERIC entries only and with fewer compile-time constants than they
// have -- the action type from the argument block within its row width (ACT = -1) and the sub-step loop (S1 = false) -- which keeps the
// build within a quarter of its time without them; `plant` is the table.
template <bool PID, bool EXT, int AW, int ACT, bool PLANT = false>
hipError_t launch_step(bool multi, hipStream_t st, const GpdParams& P, const GpdState& S, const GpdStepCfg& C,
                       const Span& T, const float* action, const float* target_pos, const float* init_pose,
                       float* obs12, float* reward, uint8_t* terminated, uint8_t* truncated, float* term_obs12, GpdDone* done,
                       const float* plant = nullptr) {
    const int64_t N = static_cast<int64_t>(C.num_envs) * C.drones_per_env;
    const int Dm = C.drones_per_env;
    const bool sized = sized_variants();
    if (T.num_steps == 1) {      // gpd_step, or a rollout of one step: the low-latency single-step kernel
        const int lanes = multi ? (kBlock / Dm) * Dm : (kBlock / 64) * C.lanes_per_wave;
        const dim3 grid(static_cast<unsigned>((N + lanes - 1) / lanes));
        // the completion word is for launches whose drones all sit in wave 0 of workgroup 0 (see the end of gpd_step_kernel)
        uint32_t* const done_flag = (done != nullptr && N <= (multi ? 64 : C.lanes_per_wave)) ? done->flag : nullptr;
        const uint32_t done_seq = done != nullptr ? done->seq : 0u;
        if (done != nullptr) done->used = done_flag != nullptr;
        if constexpr (PLANT) {
            auto go = [&](auto multi_) {
                hipLaunchKernelGGL((gpd_step_plant_kernel<PID, EXT, decltype(multi_)::value, AW, ACT, false>), grid, dim3(kBlock), 0, st, S.kin,
                                   action, S.step_counter, target_pos, static_cast<const int32_t*>(S.act_ring ? S.ring_pos : S.step_counter),
                                   static_cast<uint32_t>(S.ld), C.num_envs, C.lanes_per_wave, C.target_per_env, P, S, C, init_pose, obs12,
                                   reward, terminated, truncated, term_obs12, done_flag, done_seq, plant);
            };
            if (multi) go(Const<true>{});
            else go(Const<false>{});
            return hipGetLastError();
        } else {
            return launch_first_fit<kStepVariants, EXT, ACT>(sized, C, [&](auto I) {
                constexpr Variant v = kStepVariants[decltype(I)::value];
                hipLaunchKernelGGL((gpd_step_kernel<PID, EXT, v.multi, AW, ACT, v.s1, v.dc, v.fl, v.hi>), grid, dim3(kBlock), 0, st, S.kin, action,
                                   S.step_counter, target_pos, static_cast<const int32_t*>(S.act_ring ? S.ring_pos : S.step_counter),
                                   static_cast<uint32_t>(S.ld), C.num_envs, C.lanes_per_wave, C.target_per_env, P, S, C, init_pose, obs12,
                                   reward, terminated, truncated, term_obs12, done_flag, done_seq);
            });
        }
    }
    // Rollouts.  gpd_rollout1_kernel (no helper wave, no workgroup barrier) serves single drones and aviaries of up to 64 drones, WHOLE
    // aviaries per wave -- also where the size does not divide 64 and some lanes of every wave stay without a drone: 0.49-0.69 of the
    // compute-wave + store-wave kernel's time per step at every size from 3 to 63, half-empty waves (33 drones) included (DESIGN.md
    // section 3.2, profiles/r06_ab_wave_local_rollout.json).  Calls that keep terminal observations (conditional stores) and larger
    // aviaries go to the compute-wave + store-wave kernel, whose workgroups hold (256 / D) D drones; the two packings agree where D
    // divides 64.
    const bool roll1 = term_obs12 == nullptr && (!multi || Dm <= 64);
    const bool pow2 = Dm <= 64 && (Dm & (Dm - 1)) == 0;
    const int lanes = multi && roll1 ? 4 * ((64 / Dm) * Dm) : (multi ? (kBlock / Dm) * Dm : kBlock);
    const dim3 grid(static_cast<unsigned>((N + lanes - 1) / lanes));
    Span Tr = T;
    Tr.ring = ((!multi || pow2) && grid.x <= 2u * 256u) ? 4 : 2;   // <= 2 workgroups per CU: LDS is not what limits occupancy
    if (!roll1) {
        // multi-drone aviaries keep the run-time action-type ladder (ACT = -1: their steps are dominated by the exchange and the
        // barriers); single drones fold the action type and the sub-step count (0.891 -> 0.846 us per step), generic <AW> under the hook
        const size_t lds = static_cast<size_t>(Tr.ring) * kSlotBytes;
        auto roll = [&](auto multi_, auto act, auto s1) {
            if constexpr (PLANT)
                hipLaunchKernelGGL((gpd_rollout_plant_kernel<PID, EXT, decltype(multi_)::value, AW, decltype(act)::value, decltype(s1)::value>),
                                   grid, dim3(kRollThreads), lds, st, P, S, C, Tr, action, target_pos, init_pose, obs12, reward, terminated,
                                   truncated, term_obs12, plant);
            else
                hipLaunchKernelGGL((gpd_rollout_kernel<PID, EXT, decltype(multi_)::value, AW, decltype(act)::value, decltype(s1)::value>), grid,
                                   dim3(kRollThreads), lds, st, P, S, C, Tr, action, target_pos, init_pose, obs12, reward, terminated, truncated,
                                   term_obs12);
        };
        if (multi) roll(Const<true>{}, Const<-1>{}, Const<false>{});
        else if constexpr (PLANT) roll(Const<false>{}, Const<-1>{}, Const<false>{});
        else if (!sized) roll(Const<false>{}, Const<-1>{}, Const<false>{});
        else if (C.substeps == 1) roll(Const<false>{}, Const<ACT>{}, Const<true>{});
        else roll(Const<false>{}, Const<ACT>{}, Const<false>{});
        return hipGetLastError();
    }
    const uint32_t hot_bits = static_cast<uint32_t>(C.auto_reset != 0) | (static_cast<uint32_t>(C.init_per_env != 0) << 1) |
                              (static_cast<uint32_t>(C.target_per_env != 0) << 2);
    if constexpr (PLANT) {
        auto go = [&](auto multi_) {
            hipLaunchKernelGGL((gpd_rollout1_plant_kernel<PID, EXT, AW, ACT, false, decltype(multi_)::value>), grid, dim3(kBlock), 0, st, S.kin,
                               action, S.step_counter, target_pos, init_pose, static_cast<uint32_t>(S.ld), C.num_envs, Tr.num_steps, hot_bits,
                               P, S, C, Tr, obs12, reward, terminated, truncated, term_obs12, plant);
        };
        if (multi) go(Const<true>{});
        else go(Const<false>{});
        return hipGetLastError();
    } else {
        auto launch = [&](auto I, auto nt_obs, auto ring) {                   // entry I of kRoll1Variants
            constexpr Variant v = kRoll1Variants[decltype(I)::value];
            hipLaunchKernelGGL((gpd_rollout1_kernel<PID, EXT, AW, ACT, v.s1, v.multi, decltype(nt_obs)::value, decltype(ring)::value, v.dc, v.fl,
                                                    v.hi>),
                               grid, dim3(kBlock), 0, st, S.kin, action, S.step_counter, target_pos, init_pose, static_cast<uint32_t>(S.ld),
                               C.num_envs, Tr.num_steps, hot_bits, P, S, C, Tr, obs12, reward, terminated, truncated, term_obs12);
        };
        // The headline shape -- plain DYN, RPM actions, one sub-step, a batch that leaves one wave per SIMD -- stores its observation
        // bursts as ordinary stores: 3-4 % faster there (0.837 -> 0.803 us per step), while every other shape (larger batches, sub-step
        // loops, multi-drone aviaries) is 1-3 % faster with non-temporal ones (A/B on one box, round 2: scratch/ab.sh, scratch/ab2.sh) --
        // and only for long rollouts: the ordinary stores leave their lines to the end-of-kernel write-back, which a 20-step launch does
        // not amortise (1.14 vs 1.00 us per step).
        const bool plain_obs = N <= (1 << 17) && T.num_steps >= 48;
        // gpd_rollout_history (the action ring: it checked the shape) takes the generic entries
        return launch_first_fit<kRoll1Variants, EXT, ACT>(sized && !S.act_ring, C, [&](auto I) {
            constexpr Variant v = kRoll1Variants[decltype(I)::value];
            if constexpr (!v.sized()) {
                if (S.act_ring) return launch(I, Const<true>{}, Const<true>{});
                if constexpr (!PID && !EXT && ACT == GPD_ACT_RPM && !v.multi && v.s1)
                    if (plain_obs) return launch(I, Const<false>{}, Const<false>{});
            }
            launch(I, Const<true>{}, Const<false>{});
        });
    }
}

// gpd_plant_derive: one lane per drone.  float64 from the nominal struct's fp32 fields, one rounding per row (include/gpd.h GPD_PLANT_*;
// FP contraction is off for the unit, so `a*b + c` is two roundings in double as on the host): scales of 1.0 give the nominal fields.
__global__ __launch_bounds__(256) void gpd_plant_derive_kernel(const GpdParams P, const float* __restrict__ scales,
                                                               const uint8_t* __restrict__ env_mask, const uint32_t n, const uint32_t D,
                                                               const int64_t ld, float* __restrict__ rows) {
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (i >= n) return;
    if (env_mask && !env_mask[i / D]) return;
    double s[GPD_NUM_SCALES];
#pragma unroll
    for (int k = 0; k < GPD_NUM_SCALES; ++k) s[k] = scales[k * ld + i];
    auto put = [&](int r, double v) { rows[r * ld + i] = static_cast<float>(v); };
    const double m = s[GPD_SCALE_MASS], kf = s[GPD_SCALE_KF], ht = P.hover_thrust;
    put(GPD_PLANT_M, static_cast<double>(P.M) * m);
    put(GPD_PLANT_INV_M, static_cast<double>(P.inv_M) / m);
    put(GPD_PLANT_KF, static_cast<double>(P.KF) * kf);
    put(GPD_PLANT_GRAVITY, static_cast<double>(P.GRAVITY) * m);
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        put(GPD_PLANT_J + k, static_cast<double>(P.J[k]) * s[GPD_SCALE_IXX + k]);
        put(GPD_PLANT_J_INV + k, static_cast<double>(P.J_INV[k]) / s[GPD_SCALE_IXX + k]);
    }
    put(GPD_PLANT_KM_OVER_KF, static_cast<double>(P.km_over_kf) * s[GPD_SCALE_KM] / kf);
    put(GPD_PLANT_GND_EFF, static_cast<double>(P.gnd_eff_coeff) * s[GPD_SCALE_GND_EFF]);
    put(GPD_PLANT_DRAG, static_cast<double>(P.drag_coeff[0]) * s[GPD_SCALE_DRAG_XY]);
    put(GPD_PLANT_DRAG + 1, static_cast<double>(P.drag_coeff[1]) * s[GPD_SCALE_DRAG_XY]);
    put(GPD_PLANT_DRAG + 2, static_cast<double>(P.drag_coeff[2]) * s[GPD_SCALE_DRAG_Z]);
    put(GPD_PLANT_HOVER_THRUST, ht * m);                                       // the drone's F_h = GRAVITY/4
    put(GPD_PLANT_HOVER_RESID, static_cast<double>(P.hover_resid) * kf + (kf - m) * ht);   // KF*h32^2 - F_h, without cancellation
    put(GPD_PLANT_NORM_THRUST, ht * kf);                                       // KF*HOVER_RPM^2 of the nominal hover rpm
    put(GPD_PLANT_NORM_GAP, (m - kf) * ht);                                    // F_h - T: +0 for a nominal row
}

// argument checks + launch shared by gpd_step (K = 1) and gpd_rollout
int step_impl(const char* who, const GpdParams* params, const GpdState* state, const GpdStepCfg* cfg, const Span& T,
              const float* action, const float* target_pos, const float* init_pose, float* obs12, float* reward,
              uint8_t* terminated, uint8_t* truncated, float* term_obs12, void* stream, GpdDone* done = nullptr,
              const float* plant = nullptr) {
    auto bad = [&](int code, const char* msg) { return fail(code, (std::string(who) + ": " + msg).c_str()); };
    if (!params || !state || !cfg) return bad(GPD_EINVAL, "NULL params/state/cfg");
    if (!state->kin || !state->step_counter) return bad(GPD_EINVAL, "NULL state.kin/step_counter");
    if (const char* why = state_layout_problem(state)) return bad(GPD_EINVAL, why);
    if (!action || !obs12 || !reward || !terminated || !truncated)
        return bad(GPD_EINVAL, "NULL action/obs12/reward/terminated/truncated");
    if (cfg->num_envs <= 0 || cfg->drones_per_env <= 0 || cfg->substeps <= 0)
        return bad(GPD_EINVAL, "num_envs, drones_per_env and substeps must be positive");
    if (cfg->drones_per_env > kBlock) return bad(GPD_ERANGE, "drones_per_env > 256 is not supported");
    if (cfg->act_type < GPD_ACT_RPM || cfg->act_type > GPD_ACT_DIRECT_RPM) return bad(GPD_EINVAL, "unknown act_type");
    if (cfg->task < GPD_TASK_NONE || cfg->task > GPD_TASK_MULTIHOVER) return bad(GPD_EINVAL, "unknown task");
    if (cfg->physics_flags & ~31u) return bad(GPD_EINVAL, "unknown physics flag");
    const int64_t N = static_cast<int64_t>(cfg->num_envs) * cfg->drones_per_env;
    if (state->ld < N) return bad(GPD_EINVAL, "state.ld < num_envs*drones_per_env");
    if (N > (1LL << 26)) return bad(GPD_ERANGE, "more than 2^26 drones per launch (32-bit byte offsets)");
    const bool pid = cfg->act_type == GPD_ACT_PID || cfg->act_type == GPD_ACT_VEL || cfg->act_type == GPD_ACT_ONE_D_PID;
    if (pid && !state->pid) return bad(GPD_EINVAL, "PID action type needs state.pid");
    if (pid && params->pid_kf <= 0.0f)
        return bad(GPD_ENOTSUP, "no DSLPID controller for this airframe (CF2X/CF2P only)");
    if ((cfg->physics_flags & GPD_PHYS_DRAG) && !state->last_rpm) return bad(GPD_EINVAL, "GPD_PHYS_DRAG needs state.last_rpm");
    if (cfg->task != GPD_TASK_NONE && !target_pos) return bad(GPD_EINVAL, "task needs target_pos");
    if (cfg->auto_reset && !init_pose) return bad(GPD_EINVAL, "auto_reset needs init_pose");
    const bool multi = cfg->drones_per_env > 1;
    GpdStepCfg c = *cfg;
    if (c.lanes_per_wave == 0) c.lanes_per_wave = 64;
    if (c.lanes_per_wave != 16 && c.lanes_per_wave != 32 && c.lanes_per_wave != 64)
        return bad(GPD_EINVAL, "lanes_per_wave must be 0, 16, 32 or 64");
    const int min_lanes = multi ? (kBlock / cfg->drones_per_env) * cfg->drones_per_env : (kBlock / 64) * c.lanes_per_wave;
    if ((N + min_lanes - 1) / min_lanes > 0x7fffffffLL) return bad(GPD_ERANGE, "too many drones for one launch");
    hipStream_t st = static_cast<hipStream_t>(stream);
    const bool ext = cfg->physics_flags != 0;
    // task NONE never uses the target: hand the kernel a readable dummy so that its load section is branch-free
    if (cfg->task == GPD_TASK_NONE) { target_pos = state->kin; c.target_per_env = 0; }
    hipError_t e;
    if (plant) {     // gpd_rollout_plant: the action type from the argument block within its row width (launch_step)
#define GPD_PLANT_LAUNCH(PID_, AW_)                                                                                                  \
    (ext ? launch_step<PID_, true, AW_, -1, true>(multi, st, *params, *state, c, T, action, target_pos, init_pose, obs12, reward,     \
                                                  terminated, truncated, term_obs12, nullptr, plant)                                  \
         : launch_step<PID_, false, AW_, -1, true>(multi, st, *params, *state, c, T, action, target_pos, init_pose, obs12, reward,    \
                                                   terminated, truncated, term_obs12, nullptr, plant))
        switch (cfg->act_type) {
            case GPD_ACT_PID: e = GPD_PLANT_LAUNCH(true, 3); break;
            case GPD_ACT_VEL: e = GPD_PLANT_LAUNCH(true, 4); break;
            case GPD_ACT_ONE_D_PID: e = GPD_PLANT_LAUNCH(true, 1); break;
            case GPD_ACT_ONE_D_RPM: e = GPD_PLANT_LAUNCH(false, 1); break;
            default: e = GPD_PLANT_LAUNCH(false, 4); break;          // RPM, RAW_RPM, DIRECT_RPM
        }
#undef GPD_PLANT_LAUNCH
        if (e != hipSuccess) return hip_fail(e, who);
        return 0;
    }
#define GPD_LAUNCH(PID_, EXT_, AW_, ACT_)                                                                            \
    launch_step<PID_, EXT_, AW_, ACT_>(multi, st, *params, *state, c, T, action, target_pos, init_pose, obs12, reward, \
                                       terminated, truncated, term_obs12, done)
    switch (cfg->act_type) {
        case GPD_ACT_PID: e = ext ? GPD_LAUNCH(true, true, 3, GPD_ACT_PID) : GPD_LAUNCH(true, false, 3, GPD_ACT_PID); break;
        case GPD_ACT_VEL: e = ext ? GPD_LAUNCH(true, true, 4, GPD_ACT_VEL) : GPD_LAUNCH(true, false, 4, GPD_ACT_VEL); break;
        case GPD_ACT_ONE_D_PID:
            e = ext ? GPD_LAUNCH(true, true, 1, GPD_ACT_ONE_D_PID) : GPD_LAUNCH(true, false, 1, GPD_ACT_ONE_D_PID); break;
        case GPD_ACT_ONE_D_RPM:
            e = ext ? GPD_LAUNCH(false, true, 1, GPD_ACT_ONE_D_RPM) : GPD_LAUNCH(false, false, 1, GPD_ACT_ONE_D_RPM); break;
        case GPD_ACT_RAW_RPM:
            e = ext ? GPD_LAUNCH(false, true, 4, GPD_ACT_RAW_RPM) : GPD_LAUNCH(false, false, 4, GPD_ACT_RAW_RPM); break;
        case GPD_ACT_DIRECT_RPM:
            e = ext ? GPD_LAUNCH(false, true, 4, GPD_ACT_DIRECT_RPM) : GPD_LAUNCH(false, false, 4, GPD_ACT_DIRECT_RPM); break;
        default: e = ext ? GPD_LAUNCH(false, true, 4, GPD_ACT_RPM) : GPD_LAUNCH(false, false, 4, GPD_ACT_RPM); break;
    }
#undef GPD_LAUNCH
    if (e != hipSuccess) return hip_fail(e, who);
    return 0;
}

}  // namespace

// The DSLPID variants of the policy kernel are instantiated HERE, under this unit's scheduler (gpd_common.inc says why);
// GPD_PID_POLICY_IN_POLICY_TU (experiment / regression switch, tests/test_kernel_isa.py) moves them to policy.hip
#ifndef GPD_PID_POLICY_IN_POLICY_TU
void gpd_detail_launch_policy_pid(const GpdPolicyLaunch& a) {
    const Span& T = *static_cast<const Span*>(a.span);
    const dim3 grid(a.grid);
    hipStream_t st = static_cast<hipStream_t>(a.stream);
#define GPD_POL(AW_, ACT_, NK1_)                                                                                                   \
    do {                                                                                                                            \
        if (a.policy->activation == 1)                                                                                              \
            hipLaunchKernelGGL((gpd_rollout_policy_kernel<true, AW_, ACT_, NK1_, true>), grid, dim3(kBlock), 0, st, *a.params, *a.state, *a.cfg, T, \
                               *a.policy, a.obs12_in, a.target_pos, a.init_pose, a.actions_out, a.obs12, a.reward, a.terminated, a.truncated, a.term_obs12); \
        else                                                                                                                        \
            hipLaunchKernelGGL((gpd_rollout_policy_kernel<true, AW_, ACT_, NK1_, false>), grid, dim3(kBlock), 0, st, *a.params, *a.state, *a.cfg, T, \
                               *a.policy, a.obs12_in, a.target_pos, a.init_pose, a.actions_out, a.obs12, a.reward, a.terminated, a.truncated, a.term_obs12); \
    } while (0)
    switch (a.cfg->act_type) {
        case GPD_ACT_VEL: if (a.hist) GPD_POL(4, GPD_ACT_VEL, 5); else GPD_POL(4, GPD_ACT_VEL, 1); break;
        case GPD_ACT_PID: if (a.hist) GPD_POL(3, GPD_ACT_PID, 4); else GPD_POL(3, GPD_ACT_PID, 1); break;
        default: if (a.hist) GPD_POL(1, GPD_ACT_ONE_D_PID, 2); else GPD_POL(1, GPD_ACT_ONE_D_PID, 1); break;
    }
#undef GPD_POL
}
#endif

GPD_DBG_READER(gpd_detail_dbg_read_step)

extern "C" {

int gpd_step(const GpdParams* params, const GpdState* state, const GpdStepCfg* cfg, const float* action,
             const float* target_pos, const float* init_pose, float* obs12, float* reward, uint8_t* terminated,
             uint8_t* truncated, float* term_obs12, void* stream) {
    const Span T{1, 0, 0, 0, 2};
    return step_impl("gpd_step", params, state, cfg, T, action, target_pos, init_pose, obs12, reward, terminated,
                     truncated, term_obs12, stream);
}

int gpd_step_sync(const GpdParams* params, const GpdState* state, const GpdStepCfg* cfg, const float* action,
                  const float* target_pos, const float* init_pose, float* obs12, float* reward, uint8_t* terminated,
                  uint8_t* truncated, float* term_obs12, void* stream) {
    GpdDone done = gpd_detail_done_begin();              // (how the wait works: gpd_common.inc)
    const Span T{1, 0, 0, 0, 2};
    if (int rc = step_impl("gpd_step_sync", params, state, cfg, T, action, target_pos, init_pose, obs12, reward, terminated,
                           truncated, term_obs12, stream, done.flag != nullptr ? &done : nullptr))
        return rc;
    return gpd_detail_done_wait(done, stream, "gpd_step_sync");
}

int gpd_rollout(const GpdParams* params, const GpdState* state, const GpdStepCfg* cfg, int32_t num_steps,
                const float* actions, int64_t action_step_stride, const float* target_pos, const float* init_pose,
                float* obs12, int64_t obs_step_stride, float* reward, uint8_t* terminated, uint8_t* truncated,
                int64_t env_step_stride, float* term_obs12, void* stream) {
    if (num_steps <= 0) return fail(GPD_EINVAL, "gpd_rollout: num_steps must be positive");
    if (action_step_stride < 0 || obs_step_stride < 0 || env_step_stride < 0)
        return fail(GPD_EINVAL, "gpd_rollout: strides must be non-negative");
    const Span T{num_steps, action_step_stride, obs_step_stride, env_step_stride, 2};
    // a rollout never pushes into the action ring itself (gpd_full_obs does, after the call) -- also not when a one-step
    // rollout is routed to the single-step kernel
    GpdState no_ring;
    if (state) { no_ring = *state; no_ring.act_ring = nullptr; }
    return step_impl("gpd_rollout", params, state ? &no_ring : nullptr, cfg, T, actions, target_pos, init_pose, obs12, reward,
                     terminated, truncated, term_obs12, stream);
}

int gpd_rollout_history(const GpdParams* params, const GpdState* state, const GpdStepCfg* cfg, int32_t num_steps,
                        const float* actions, int64_t action_step_stride, const float* target_pos, const float* init_pose,
                        float* obs12, int64_t obs_step_stride, float* reward, uint8_t* terminated, uint8_t* truncated,
                        int64_t env_step_stride, void* stream) {
    if (num_steps <= 0) return fail(GPD_EINVAL, "gpd_rollout_history: num_steps must be positive");
    if (action_step_stride < 0 || obs_step_stride < 0 || env_step_stride < 0)
        return fail(GPD_EINVAL, "gpd_rollout_history: strides must be non-negative");
    if (!state || !state->act_ring || !state->ring_pos || state->hist_len <= 0)
        return fail(GPD_EINVAL, "gpd_rollout_history: state has no action ring (act_ring / ring_pos / hist_len)");
    if (cfg && cfg->drones_per_env > 64)
        return fail(GPD_ENOTSUP, "gpd_rollout_history: aviaries of up to 64 drones (use gpd_rollout + gpd_full_obs otherwise)");
    const Span T{num_steps, action_step_stride, obs_step_stride, env_step_stride, 2};
    return step_impl("gpd_rollout_history", params, state, cfg, T, actions, target_pos, init_pose, obs12, reward, terminated,
                     truncated, nullptr, stream);
}

int gpd_plant_derive(const GpdParams* nominal, const float* scales, const uint8_t* env_mask, int32_t num_envs, int32_t drones_per_env,
                     int64_t ld, float* rows, void* stream) {
    if (!nominal || !scales || !rows) return fail(GPD_EINVAL, "gpd_plant_derive: NULL nominal/scales/rows");
    if (num_envs <= 0 || drones_per_env <= 0) return fail(GPD_EINVAL, "gpd_plant_derive: num_envs and drones_per_env must be positive");
    const int64_t n = static_cast<int64_t>(num_envs) * drones_per_env;
    if (ld < n) return fail(GPD_EINVAL, "gpd_plant_derive: ld < num_envs*drones_per_env");
    if (n > (1LL << 26)) return fail(GPD_ERANGE, "gpd_plant_derive: more than 2^26 drones");
    if (reinterpret_cast<uintptr_t>(rows) & 15u) return fail(GPD_EINVAL, "gpd_plant_derive: rows must be 16-byte aligned");
    hipLaunchKernelGGL(gpd_plant_derive_kernel, dim3(static_cast<unsigned>((n + 255) / 256)), dim3(256), 0, static_cast<hipStream_t>(stream),
                       *nominal, scales, env_mask, static_cast<uint32_t>(n), static_cast<uint32_t>(drones_per_env), ld, rows);
    if (hipError_t e = hipGetLastError(); e != hipSuccess) return hip_fail(e, "gpd_plant_derive");
    return 0;
}

int gpd_rollout_plant(const GpdParams* params, const GpdState* state, const GpdStepCfg* cfg, int32_t num_steps,
                      const float* actions, int64_t action_step_stride, const float* target_pos, const float* init_pose,
                      float* obs12, int64_t obs_step_stride, float* reward, uint8_t* terminated, uint8_t* truncated,
                      int64_t env_step_stride, float* term_obs12, const float* plant_rows, void* stream) {
    if (num_steps <= 0) return fail(GPD_EINVAL, "gpd_rollout_plant: num_steps must be positive");
    if (action_step_stride < 0 || obs_step_stride < 0 || env_step_stride < 0)
        return fail(GPD_EINVAL, "gpd_rollout_plant: strides must be non-negative");
    if (!plant_rows) return fail(GPD_EINVAL, "gpd_rollout_plant: NULL plant_rows");
    if (reinterpret_cast<uintptr_t>(plant_rows) & 15u) return fail(GPD_EINVAL, "gpd_rollout_plant: plant_rows must be 16-byte aligned");
    if (state && state->dw_force)
        return fail(GPD_ENOTSUP, "gpd_rollout_plant: state.dw_force (downwash computed outside the kernel) is not served by the plant path");
    const Span T{num_steps, action_step_stride, obs_step_stride, env_step_stride, 2};
    GpdState no_ring;                                    // (as gpd_rollout: gpd_full_obs pushes the actions after the call)
    if (state) { no_ring = *state; no_ring.act_ring = nullptr; }
    return step_impl("gpd_rollout_plant", params, state ? &no_ring : nullptr, cfg, T, actions, target_pos, init_pose, obs12, reward,
                     terminated, truncated, term_obs12, stream, nullptr, plant_rows);
}

}  // extern "C"

