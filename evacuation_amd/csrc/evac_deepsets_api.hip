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

namespace {

using evac_host::handle_fail;

// The checks the two entries share: the thirteen tensors as evac_policy_rollout makes them, then the encoder's.
int check_networks(evac_handle_t h, const std::string& w, const evac_host::HandleView& v, const evac_mlp_policy_t* policy,
                   const evac_deepsets_t* encoder, evac::PolicyArgs& a, evac::DeepSetsArgs& da) {
    if (!policy) return handle_fail(h, EVAC_ERR_INVALID_ARGUMENT, w + ": policy is NULL");
    if (!encoder) return handle_fail(h, EVAC_ERR_INVALID_ARGUMENT, w + ": encoder is NULL");
    evac::PolicyArgs pa{};                             // (`a` and `da` are written only once every check has passed)
    if (const std::string why = mlp_policy_check(*policy, v.p.obs_dim, pa); !why.empty())
        return handle_fail(h, EVAC_ERR_INVALID_ARGUMENT, w + why);
    const evac_deepsets_t& S = *encoder;
    if (!S.phi_w1 || !S.phi_b1 || !S.phi_w2 || !S.phi_b2 || !S.rho_w || !S.rho_b)
        return handle_fail(h, EVAC_ERR_INVALID_ARGUMENT, w + ": a tensor pointer of the encoder is NULL");
    if (S.hidden != evac::kSetHidden)
        return handle_fail(h, EVAC_ERR_INVALID_ARGUMENT, w + ": the encoder's hidden must be " + std::to_string(evac::kSetHidden));
    // (the gravity observation's 6 floats are no whole number of rows for any N >= 5, and no set for the others)
    if (v.p.obs_pos == EVAC_POS_GRAV || S.set_elem_dim < 1 || S.set_elem_dim > evac::kSetMaxElemDim ||
        (int64_t)S.set_elem_dim * (v.p.n_ped + 2) != (int64_t)v.p.obs_dim)
        return handle_fail(h, EVAC_ERR_INVALID_ARGUMENT, w + ": set_elem_dim " + std::to_string(S.set_elem_dim) + " x (" +
                                                             std::to_string(v.p.n_ped) + " + 2) elements is not the observation's " +
                                                             std::to_string(v.p.obs_dim) + " floats (a Box observation is needed)");
    if ((uintptr_t)S.rho_w & 15u) return handle_fail(h, EVAC_ERR_INVALID_ARGUMENT, w + ": rho_w must be 16-byte aligned");
    a = pa;
    da = evac::DeepSetsArgs{S.phi_w1, S.phi_b1, S.phi_w2, S.phi_b2, S.rho_w, S.rho_b, (int)S.set_elem_dim};
    return EVAC_OK;
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
    if (v.p.n_ped > evac::kWave)
        return handle_fail(h, EVAC_ERR_UNSUPPORTED, w + ": rooms of more than 64 pedestrians are not supported (one wave per env)");
    if (n_steps < 1) return handle_fail(h, EVAC_ERR_INVALID_ARGUMENT, w + ": n_steps must be >= 1");
    if (!next_obs || !next_done || !obs_out || !actions_out || !logprob_out || !value_out || !reward_out || !done_out || !next_value_out)
        return handle_fail(h, EVAC_ERR_INVALID_ARGUMENT, w + ": every output buffer but final_stats / norm_state must be non-NULL");
    evac::PolicyArgs a{};
    evac::DeepSetsArgs da{};
    if (const int rc = check_networks(h, w, v, policy, encoder, a, da); rc != EVAC_OK) return rc;
    if ((uintptr_t)actions_out & 7u) return handle_fail(h, EVAC_ERR_INVALID_ARGUMENT, w + ": actions_out must be 8-byte aligned");
    if (const int st = evac_host::handle_settle(h, (hipStream_t)stream); st != EVAC_OK) return st;
    DeviceGuard g(v.device);
    a.next_obs = next_obs; a.next_done = next_done; a.obs_out = obs_out; a.actions_out = actions_out; a.logprob_out = logprob_out;
    a.value_out = value_out; a.reward_out = reward_out; a.done_out = done_out; a.next_value_out = next_value_out;
    a.final_stats = final_stats;
    const evac::NormArgs na{norm_state, gamma, obs_clip, reward_clip, epsilon};
    const bool norm = norm_state != nullptr, def = v.default_cfg;
    const auto fn = EVAC_PICK_BOOL2(evac::k_policy_rollout_deepsets, norm, def);
    const int per_block = evac::PolicyFamily::kEnvsPerBlock;
    hipLaunchKernelGGL(fn, dim3((unsigned)((v.p.n_envs + per_block - 1) / per_block)), dim3(evac::PolicyFamily::kBlock), 0,
                       (hipStream_t)stream, v.p, (int)n_steps, a, na, da);
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
    if (!progress || !episodes_out) return handle_fail(h, EVAC_ERR_INVALID_ARGUMENT, w + ": progress / episodes_out is NULL");
    if (n_episodes < 1 || max_steps < 1) return handle_fail(h, EVAC_ERR_INVALID_ARGUMENT, w + ": n_episodes and max_steps must be >= 1");
    if ((uintptr_t)progress & 15u) return handle_fail(h, EVAC_ERR_INVALID_ARGUMENT, w + ": progress must be 16-byte aligned");
    evac::PolicyArgs a{};
    evac::DeepSetsArgs da{};
    if (const int rc = check_networks(h, w, v, policy, encoder, a, da); rc != EVAC_OK) return rc;
    if (v.p.n_ped > evac::kWave)
        return handle_fail(h, EVAC_ERR_UNSUPPORTED, w + ": rooms of more than 64 pedestrians are not supported (one wave per env)");
    if (const int st = evac_host::handle_settle(h, (hipStream_t)stream); st != EVAC_OK) return st;
    DeviceGuard g(v.device);
    const evac::EvalArgs ev{(int4*)progress, episodes_out, norm_state, (int)n_episodes, (int)max_steps,
                            agent == EVAC_AGENT_POLICY_SAMPLE ? 1 : 0, obs_clip, epsilon, 0.0f, 0.0f};
    const bool norm = norm_state != nullptr, def = v.default_cfg;
    const auto fn = EVAC_PICK_BOOL2(evac::k_policy_evaluate_deepsets, norm, def);
    const int per_block = evac::PolicyFamily::kEnvsPerBlock;
    hipLaunchKernelGGL(fn, dim3((unsigned)((v.p.n_envs + per_block - 1) / per_block)), dim3(evac::PolicyFamily::kBlock), 0,
                       (hipStream_t)stream, v.p, a, ev, da);
    return evac_host::handle_check_launch(h, w.c_str());
}

}  // extern "C"
