// Host side of the transformer leader (include/evac.h: evac_policy_rollout_transformer, evac_policy_evaluate_transformer; kernels
// in evac_transformer.h): the encoder's blocks beside the actor-critic's thirteen tensors.  The two entries' bodies -- the checks
// in their order, the handle, the launch -- are evac_handle_host.h's encoder_rollout / encoder_evaluate, which
// evac_deepsets_api.hip shares; this unit holds what is the attention encoder's own: its limits and its kernels (its check: evac_transformer_env_host.h).
#include <hip/hip_runtime.h>

#include <cstddef>
#include <cstdint>
#include <string>

#define EVAC_TEMPLATE_KERNELS_ONLY      // (evac_device.h: its plain kernels live in evac_api.hip)
#include "evac_transformer.h"
#include "evac_handle_host.h"
#include "evac_host.h"
#include "evac_transformer_env_host.h"

static_assert(sizeof(evac::Params) + 8 + sizeof(evac::PolicyArgs) + sizeof(evac::NormArgs) + sizeof(evac::TransformerArgs) <= 4096,
              "k_policy_rollout_transformer: arguments beyond the kernel-argument segment");
static_assert(sizeof(evac::PolicyFamily::Smem) + sizeof(evac::PolicySmem<false>) + sizeof(evac::EvalSmem) +
                  sizeof(evac::TransformerSmem) <= 160 * 1024, "the transformer kernels' LDS beyond a CU's 160 KiB");
namespace {

// evac_handle_host.h's trait of an encoder: the attention encoder's check (evac_transformer_env_host.h), this unit's names and
// kernels.
struct TransformerEncoder : TransformerEncoderHost {
    static constexpr const char* kRollout = "evac_policy_rollout_transformer";
    static constexpr const char* kEvaluate = "evac_policy_evaluate_transformer";
    static auto rollout_kernel(bool norm, bool def) { return EVAC_PICK_BOOL2(evac::k_policy_rollout_transformer, norm, def); }
    static auto evaluate_kernel(bool norm, bool def) { return EVAC_PICK_BOOL2(evac::k_policy_evaluate_transformer, norm, def); }
};

}  // namespace

extern "C" {

int evac_policy_rollout_transformer(evac_handle_t h, int32_t n_steps, const evac_mlp_policy_t* policy, float* next_obs, float* next_done,
                                    float* obs_out, float* actions_out, float* logprob_out, float* value_out, float* reward_out,
                                    float* done_out, float* next_value_out, evac_episode_stats_t* final_stats, double* norm_state,
                                    float gamma, float obs_clip, float reward_clip, float epsilon, const evac_transformer_t* encoder,
                                    void* stream) {
    return encoder_rollout<TransformerEncoder>(h, n_steps, policy,
                                               collect_outputs(next_obs, next_done, obs_out, actions_out, logprob_out, value_out,
                                                               reward_out, done_out, next_value_out, final_stats),
                                               evac::NormArgs{norm_state, gamma, obs_clip, reward_clip, epsilon}, encoder, stream);
}

int evac_policy_evaluate_transformer(evac_handle_t h, int32_t agent, const evac_mlp_policy_t* policy, int32_t n_episodes,
                                     int32_t max_steps, int32_t* progress, evac_episode_stats_t* episodes_out, const double* norm_state,
                                     float obs_clip, float epsilon, const evac_transformer_t* encoder, void* stream) {
    return encoder_evaluate<TransformerEncoder>(h, agent, policy, n_episodes, max_steps, progress, episodes_out, norm_state, obs_clip,
                                                epsilon, encoder, stream);
}

}  // extern "C"
