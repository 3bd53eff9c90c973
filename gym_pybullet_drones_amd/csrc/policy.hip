// policy.hip -- gpd_rollout_policy
#include "gpd_common.inc"
#include "policy_kernel.inc"

#ifdef GPD_PID_POLICY_IN_POLICY_TU
void gpd_detail_launch_policy_pid(const GpdPolicyLaunch& a) { launch_policy<true>(a); }
#endif

GPD_DBG_READER(gpd_detail_dbg_read_policy)

extern "C" {

int gpd_rollout_policy(const GpdParams* params, const GpdState* state, const GpdStepCfg* cfg, const GpdPolicy* policy,
                       int32_t num_steps, const float* obs12_in, const float* target_pos, const float* init_pose,
                       float* actions_out, float* obs12, int64_t obs_step_stride, float* reward, uint8_t* terminated,
                       uint8_t* truncated, int64_t env_step_stride, const float* noise, const float* action_std, float* mean_out,
                       float* term_obs12, void* stream) {
    const Refuse bad{"gpd_rollout_policy"};
    if ((noise != nullptr) != (action_std != nullptr)) return bad(GPD_EINVAL, "noise and action_std come together");
    if (mean_out && !noise) return bad(GPD_EINVAL, "mean_out is written by the sampling kernels only (pass noise)");
    if (!params || !state || !cfg || !policy) return bad(GPD_EINVAL, "NULL params/state/cfg/policy");
    if (int rc = check_state(bad, state)) return rc;
    if (!obs12_in || !obs12 || !reward || !terminated || !truncated) return bad(GPD_EINVAL, "NULL obs12_in/obs12/reward/terminated/truncated");
    if (!policy->w1 || !policy->b1 || !policy->w2 || !policy->b2 || !policy->w3 || !policy->b3) return bad(GPD_EINVAL, "NULL policy weights");
    if (int rc = check_steps(bad, num_steps, obs_step_stride, env_step_stride)) return rc;
    // what the kernel serves, in front of the shared checks (a drones_per_env or act_type outside it answers GPD_ENOTSUP)
    if (cfg->drones_per_env != 1) return bad(GPD_ENOTSUP, "single-drone aviaries only (drones_per_env == 1)");
    if (cfg->act_type < GPD_ACT_RPM || cfg->act_type > GPD_ACT_ONE_D_PID) return bad(GPD_ENOTSUP, "one of the five ActionTypes (RPM, PID, VEL, ONE_D_RPM, ONE_D_PID)");
    if (int rc = check_positive(bad, cfg)) return rc;
    if (int rc = check_ranges(bad, cfg)) return rc;
    if (int rc = check_flags(bad, cfg)) return rc;
    if (policy->hidden != kPolHidden) return bad(GPD_ENOTSUP, "hidden must be 64");
    if (policy->activation != 0 && policy->activation != 1) return bad(GPD_EINVAL, "activation must be 0 (tanh) or 1 (relu)");
    const int64_t N = cfg->num_envs;
    if (int rc = check_extent(bad, N, state->ld)) return rc;
    if (int rc = check_needs(bad, params, state, cfg, target_pos, init_pose)) return rc;
    const bool pid = cfg->act_type == GPD_ACT_PID || cfg->act_type == GPD_ACT_VEL || cfg->act_type == GPD_ACT_ONE_D_PID;
    const int A = (cfg->act_type == GPD_ACT_RPM || cfg->act_type == GPD_ACT_VEL) ? 4 : (cfg->act_type == GPD_ACT_PID ? 3 : 1);
    const int cap = 16 * pol_nk1(A, true) - 12;                       // history features the kernel's registers hold
    const bool hist = policy->in_dim != 12;
    if (hist) {
        if (!state->act_ring || !state->ring_pos || state->hist_len <= 0) return bad(GPD_EINVAL, "in_dim > 12 needs the action ring of state");
        if (policy->in_dim != 12 + state->hist_len * A) return bad(GPD_ENOTSUP, "in_dim must be 12 or 12 + hist_len*act_dim");
        if (state->hist_len * A > cap) return bad(GPD_ENOTSUP, "history too long for the in-kernel policy (17 actions of 4 or 3 floats, 20 of 1)");
    } else if (state->act_ring && (!state->ring_pos || state->hist_len <= 0)) {
        return bad(GPD_EINVAL, "state.act_ring without ring_pos / hist_len");
    }
    GpdStepCfg c = *cfg;
    dummy_target(c, target_pos, state->kin);
    const Span T{num_steps, 0, obs_step_stride, env_step_stride, 2};
    const unsigned grid = blocks_for(N, kBlock);
    const GpdPolicyLaunch a{params, state, &c, &T, policy, obs12_in, target_pos, init_pose, actions_out, obs12, reward, terminated,
                            truncated, stream, grid, hist ? 1 : 0, term_obs12};
    if (noise) {                 // sampling: the RPM action types (the ones examples/learn.py and the reference's learn.py train)
        if (pid) return bad(GPD_ENOTSUP, "sampling (noise) is implemented for ActionType.RPM and ONE_D_RPM");
        policy_variant<false>(cfg->act_type, hist, policy->activation == 1, [&](auto aw, auto act, auto nk1, auto relu) {
            constexpr int AW = decltype(aw)::value;
            const float4 sd = make_float4(action_std[0], AW > 1 ? action_std[1] : 0.0f, AW > 2 ? action_std[2] : 0.0f,
                                          AW > 3 ? action_std[3] : 0.0f);
            hipLaunchKernelGGL((gpd_rollout_policy_noise_kernel<AW, decltype(act)::value, decltype(nk1)::value, decltype(relu)::value>),
                               dim3(grid), dim3(kBlock), 0, static_cast<hipStream_t>(stream), *params, *state, c, T, *policy, obs12_in,
                               target_pos, init_pose, actions_out, obs12, reward, terminated, truncated, noise, mean_out, sd, term_obs12);
        });
    } else if (pid) {
        gpd_detail_launch_policy_pid(a);         // (instantiated in the main unit, see GpdPolicyLaunch)
    } else {
        launch_policy<false>(a);
    }
    return launched(bad.who);
}

}  // extern "C"

