// Host side of a population of deep-sets leaders (include/evac.h: evac_policy_rollout_population_deepsets,
// evac_deepsets_population_workspace_bytes, evac_deepsets_update_population; kernels in evac_deepsets_population.h and, for the
// three launches in the middle of a step, evac_population.h's through evac_population_host.h's launch functions).  The unit names
// its kernels and traits; the bodies are shared: collection is evac_handle_host.h's encoder_rollout with the learners' shares,
// the sizer and the update are evac_encoder_population_host.h's over SetGrad and SetAdam.
#include <hip/hip_runtime.h>

#include <cstddef>
#include <cstdint>
#include <string>

#define EVAC_TEMPLATE_KERNELS_ONLY      // (evac_device.h: its plain kernels live in evac_api.hip)
#include "evac_deepsets_population.h"
#include "evac_deepsets_adam_host.h"
#include "evac_deepsets_host.h"
#include "evac_encoder_population_host.h"
#include "evac_handle_host.h"
#include "evac_host.h"

static_assert(sizeof(evac::Params) + 8 + sizeof(evac::PolicyArgs) + sizeof(evac::NormArgs) + sizeof(evac::PopulationArgs) +
                      sizeof(evac::DeepSetsArgs) + sizeof(evac::DeepSetsStrides) <= 4096,
              "k_collect_population_deepsets: arguments beyond the kernel-argument segment");

namespace evac {
void deepsets_population_launch_collect(const evac_host::HandleView& v, int n_steps, const PolicyArgs& a, const NormArgs& na,
                                        int n_learners, const PopulationArgs& q, const DeepSetsArgs& ea, const DeepSetsStrides& dq,
                                        hipStream_t stream) {
    const auto fn = EVAC_PICK_BOOL2(k_collect_population_deepsets, na.state != nullptr, v.default_cfg);
    hipLaunchKernelGGL(fn, dim3((unsigned)(n_learners * q.wgs)), dim3(PolicyFamily::kBlock), 0, stream, v.p, n_steps, a, na, q, ea, dq);
}
}  // namespace evac

namespace {

// evac_handle_host.h's trait of an encoder, for the population's collection entry (the lone kernels are evac_deepsets_api.hip's)
struct DeepSetsPopulationEncoder : DeepSetsEncoderHost {
    static constexpr const char* kRollout = "evac_policy_rollout_population_deepsets";
};
// ... and its learners: their shares of the handle's envs and the strides of their 19 tensors (evac_deepsets_host.h), the launch
struct DeepSetsLearners : DeepSetsLearnerShares {
    void launch(const evac_host::HandleView& v, int n_steps, const evac::PolicyArgs& a, const evac::NormArgs& na,
                const evac::DeepSetsArgs& ea, hipStream_t S) const {
        evac::deepsets_population_launch_collect(v, n_steps, a, na, n_learners, q, ea, dq, S);
    }
};

}  // namespace

extern "C" {

int evac_policy_rollout_population_deepsets(evac_handle_t h, int32_t n_learners, const evac_mlp_policy_t* policy,
                                            const evac_mlp_policy_strides_t* strides, const evac_deepsets_t* encoder,
                                            const evac_deepsets_strides_t* enc_strides, int32_t n_steps, float* next_obs,
                                            float* next_done, float* obs_out, float* actions_out, float* logprob_out, float* value_out,
                                            float* reward_out, float* done_out, float* next_value_out, evac_episode_stats_t* final_stats,
                                            double* norm_state, float gamma, float obs_clip, float reward_clip, float epsilon,
                                            void* stream) {
    return encoder_rollout<DeepSetsPopulationEncoder>(h, n_steps, policy,
                                                      collect_outputs(next_obs, next_done, obs_out, actions_out, logprob_out, value_out,
                                                                      reward_out, done_out, next_value_out, final_stats),
                                                      evac::NormArgs{norm_state, gamma, obs_clip, reward_clip, epsilon}, encoder, stream,
                                                      DeepSetsLearners{{n_learners, strides, enc_strides}});
}

int64_t evac_deepsets_population_workspace_bytes(int32_t obs_dim, int64_t n_minibatch, int32_t n_learners) {
    return encoder_population_workspace_bytes<SetGrad>(obs_dim, n_minibatch, n_learners);
}

int evac_deepsets_update_population(int32_t n_learners, const evac_mlp_policy_t* policy, const evac_deepsets_t* encoder,
                                    const evac_mlp_policy_grads_t* params, const evac_deepsets_grads_t* enc_params,
                                    const evac_mlp_policy_grads_t* grads, const evac_deepsets_grads_t* enc_grads,
                                    const evac_mlp_policy_strides_t* param_strides, const evac_deepsets_strides_t* enc_param_strides,
                                    const evac_mlp_policy_strides_t* grad_strides, const evac_deepsets_strides_t* enc_grad_strides,
                                    const evac_mlp_policy_strides_t* moment_strides, const evac_deepsets_strides_t* enc_moment_strides,
                                    int64_t header_stride_bytes, const evac_rpo_loss_config_t* loss_cfg,
                                    const evac_adam_config_t* adam_cfg, const evac_deepsets_adam_state_t* state, int64_t batch_size,
                                    const float* b_obs, const float* b_actions, const float* b_logprobs, const float* b_advantages,
                                    const float* b_returns, const float* b_values, int64_t learner_batch_size, int64_t n_minibatch,
                                    int32_t n_epochs, const int64_t* perms, const float* rpo_noise, const uint64_t* seeds,
                                    const uint64_t* first_draw_counters, int32_t use_target_kl, double target_kl, float* stats_out,
                                    void* workspace, void* stream) {
    return encoder_update_population<SetGrad, SetAdam>(
        evac::k_adam_set_population, n_learners, policy, encoder, params, enc_params, grads, enc_grads, param_strides, enc_param_strides,
        grad_strides, enc_grad_strides, moment_strides, enc_moment_strides, header_stride_bytes, loss_cfg, adam_cfg, state, batch_size,
        b_obs, b_actions, b_logprobs, b_advantages, b_returns, b_values, learner_batch_size, n_minibatch, n_epochs, perms, rpo_noise,
        seeds, first_draw_counters, use_target_kl, target_kl, stats_out, workspace, stream);
}

}  // extern "C"
