// Host side of the deep-sets leader (include/evac.h: evac_policy_rollout_deepsets, evac_policy_evaluate_deepsets; kernels in
// evac_deepsets.h): evac_policy_rollout's / evac_policy_evaluate's checks and launch with the encoder's six tensors beside the
// actor-critic's thirteen.  The handle is reached through evac_handle_host.h.  Every refusal before the first HIP call, no device
// allocation, no synchronisation: one kernel on the caller's stream, capturable.
#include <hip/hip_runtime.h>

#include <cstddef>
#include <cstdint>
#include <string>

#define EVAC_TEMPLATE_KERNELS_ONLY      // (evac_device.h: its plain kernels live in evac_api.hip)
#include "evac_deepsets.h"
#include "evac_handle_host.h"
#include "evac_host.h"

static_assert(sizeof(evac::Params) + 8 + sizeof(evac::PolicyArgs) + sizeof(evac::NormArgs) + sizeof(evac::DeepSetsArgs) <= 4096,
              "k_policy_rollout_deepsets: arguments beyond the kernel-argument segment");
static_assert(sizeof(evac::PolicyFamily::Smem) + sizeof(evac::PolicySmem<false>) + sizeof(evac::EvalSmem) + sizeof(evac::DeepSetsSmem) <=
                  160 * 1024, "the deep-sets kernels' LDS beyond a CU's 160 KiB");

static_assert(evac::kSetHidden == kSetEncoderHidden && evac::kSetMaxElemDim == kSetEncoderMaxElemDim,
              "deepsets_check: the widths the deep-sets kernels take");

namespace {

using evac_host::handle_fail;

// The checks the two entries share: the thirteen tensors as evac_policy_rollout makes them (into `a`), then the encoder's.
// The text that follows the entry's name, or empty.
std::string check_networks(const evac::Params& p, const evac_mlp_policy_t* policy, const evac_deepsets_t* encoder, evac::PolicyArgs& a,
                           evac::DeepSetsArgs& da) {
    if (!policy) return ": policy is NULL";
    if (!encoder) return ": encoder is NULL";
    if (const std::string why = mlp_policy_check(*policy, p.obs_dim, a); !why.empty()) return why;
    const evac_deepsets_t& S = *encoder;
    // (the gravity observation's 6 floats are no whole number of rows for any N >= 5, and no set for the others)
    const bool rows_fit = p.obs_pos != EVAC_POS_GRAV && (int64_t)S.set_elem_dim * (p.n_ped + 2) == (int64_t)p.obs_dim;
    da = evac::DeepSetsArgs{S.phi_w1, S.phi_b1, S.phi_w2, S.phi_b2, S.rho_w, S.rho_b, (int)S.set_elem_dim};
    return deepsets_check(S, p.obs_dim, p.n_ped, rows_fit);
}

}  // namespace

extern "C" {

int evac_policy_rollout_deepsets(evac_handle_t h, int32_t n_steps, const evac_mlp_policy_t* policy, float* next_obs, float* next_done,
                                 float* obs_out, float* actions_out, float* logprob_out, float* value_out, float* reward_out,
                                 float* done_out, float* next_value_out, evac_episode_stats_t* final_stats, double* norm_state,
                                 float gamma, float obs_clip, float reward_clip, float epsilon, const evac_deepsets_t* encoder,
                                 void* stream) {
    const std::string w = "evac_policy_rollout_deepsets";
    evac_host::HandleView v;
    if (const int rc = evac_host::handle_begin(h, w.c_str(), &v); rc != EVAC_OK) return rc;
    std::string why = one_wave_check(v.p);
    if (!why.empty()) return handle_fail(h, EVAC_ERR_UNSUPPORTED, w + why);
    evac::PolicyArgs a = collect_outputs(next_obs, next_done, obs_out, actions_out, logprob_out, value_out, reward_out, done_out,
                                         next_value_out, final_stats);
    evac::DeepSetsArgs da{};
    why = collect_check(n_steps, a, false, policy);    // (the first refusal in the entry's order of checks)
    if (why.empty()) why = check_networks(v.p, policy, encoder, a, da);
    if (why.empty()) why = collect_aligned(a);
    if (!why.empty()) return handle_fail(h, EVAC_ERR_INVALID_ARGUMENT, w + why);
    if (const int st = evac_host::handle_settle(h, (hipStream_t)stream); st != EVAC_OK) return st;
    DeviceGuard g(v.device);
    const evac::NormArgs na{norm_state, gamma, obs_clip, reward_clip, epsilon};
    const bool norm = norm_state != nullptr, def = v.default_cfg;
    const auto fn = EVAC_PICK_BOOL2(evac::k_policy_rollout_deepsets, norm, def);
    hipLaunchKernelGGL(fn, dim3((unsigned)policy_wgs(v.p.n_envs)), dim3(evac::PolicyFamily::kBlock), 0, (hipStream_t)stream, v.p,
                       (int)n_steps, a, na, da);
    return evac_host::handle_check_launch(h, w.c_str());
}

int evac_policy_evaluate_deepsets(evac_handle_t h, int32_t agent, const evac_mlp_policy_t* policy, int32_t n_episodes, int32_t max_steps,
                                  int32_t* progress, evac_episode_stats_t* episodes_out, const double* norm_state, float obs_clip,
                                  float epsilon, const evac_deepsets_t* encoder, void* stream) {
    const std::string w = "evac_policy_evaluate_deepsets";
    evac_host::HandleView v;
    if (const int rc = evac_host::handle_begin(h, w.c_str(), &v); rc != EVAC_OK) return rc;
    if (agent == EVAC_AGENT_VACUUM_CLEANER)
        return handle_fail(h, EVAC_ERR_INVALID_ARGUMENT, w + ": the scripted agent has no network (use evac_policy_evaluate)");
    if (agent != EVAC_AGENT_POLICY_MEAN && agent != EVAC_AGENT_POLICY_SAMPLE)
        return handle_fail(h, EVAC_ERR_INVALID_ARGUMENT, w + ": unknown agent " + std::to_string(agent));
    evac::EvalArgs ev{};
    evac::PolicyArgs a{};
    evac::DeepSetsArgs da{};
    std::string why = evaluate_check(agent, n_episodes, max_steps, progress, episodes_out, norm_state, obs_clip, epsilon, ev);
    if (why.empty()) why = check_networks(v.p, policy, encoder, a, da);
    if (!why.empty()) return handle_fail(h, EVAC_ERR_INVALID_ARGUMENT, w + why);
    if (!(why = one_wave_check(v.p)).empty()) return handle_fail(h, EVAC_ERR_UNSUPPORTED, w + why);
    if (const int st = evac_host::handle_settle(h, (hipStream_t)stream); st != EVAC_OK) return st;
    DeviceGuard g(v.device);
    const bool norm = norm_state != nullptr, def = v.default_cfg;
    const auto fn = EVAC_PICK_BOOL2(evac::k_policy_evaluate_deepsets, norm, def);
    hipLaunchKernelGGL(fn, dim3((unsigned)policy_wgs(v.p.n_envs)), dim3(evac::PolicyFamily::kBlock), 0, (hipStream_t)stream, v.p, a, ev,
                       da);
    return evac_host::handle_check_launch(h, w.c_str());
}

}  // extern "C"
