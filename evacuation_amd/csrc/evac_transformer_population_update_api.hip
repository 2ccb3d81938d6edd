// Host side of the update of a population of transformer leaders (include/evac.h: evac_transformer_population_workspace_bytes,
// evac_transformer_update_population; kernels in evac_transformer_population_train.h and evac_transformer_train.h and, for the
// three launches in the middle of a step, evac_population.h's through evac_population_host.h's launch functions).  The unit names
// its kernel and traits; the sizer's and the update's bodies are evac_encoder_population_host.h's over TfGrad and TfAdam.
#include <hip/hip_runtime.h>

#include <cstddef>
#include <cstdint>

#include "evac_transformer_population_train.h"
#include "evac_transformer_adam_host.h"
#include "evac_encoder_population_host.h"

extern "C" {

int64_t evac_transformer_population_workspace_bytes(int32_t obs_dim, int64_t n_minibatch, int32_t n_learners) {
    return encoder_population_workspace_bytes<TfGrad>(obs_dim, n_minibatch, n_learners);
}

int evac_transformer_update_population(int32_t n_learners, const evac_mlp_policy_t* policy, const evac_transformer_t* encoder,
                                       const evac_mlp_policy_grads_t* params, const evac_transformer_grads_t* enc_params,
                                       const evac_mlp_policy_grads_t* grads, const evac_transformer_grads_t* enc_grads,
                                       const evac_mlp_policy_strides_t* param_strides, const evac_transformer_strides_t* enc_param_strides,
                                       const evac_mlp_policy_strides_t* grad_strides, const evac_transformer_strides_t* enc_grad_strides,
                                       const evac_mlp_policy_strides_t* moment_strides, const evac_transformer_strides_t* enc_moment_strides,
                                       int64_t header_stride_bytes, const evac_rpo_loss_config_t* loss_cfg,
                                       const evac_adam_config_t* adam_cfg, const evac_transformer_adam_state_t* state, int64_t batch_size,
                                       const float* b_obs, const float* b_actions, const float* b_logprobs, const float* b_advantages,
                                       const float* b_returns, const float* b_values, int64_t learner_batch_size, int64_t n_minibatch,
                                       int32_t n_epochs, const int64_t* perms, const float* rpo_noise, const uint64_t* seeds,
                                       const uint64_t* first_draw_counters, int32_t use_target_kl, double target_kl, float* stats_out,
                                       void* workspace, void* stream) {
    return encoder_update_population<TfGrad, TfAdam>(
        evac::k_adam_tf_population, n_learners, policy, encoder, params, enc_params, grads, enc_grads, param_strides, enc_param_strides,
        grad_strides, enc_grad_strides, moment_strides, enc_moment_strides, header_stride_bytes, loss_cfg, adam_cfg, state, batch_size,
        b_obs, b_actions, b_logprobs, b_advantages, b_returns, b_values, learner_batch_size, n_minibatch, n_epochs, perms, rpo_noise,
        seeds, first_draw_counters, use_target_kl, target_kl, stats_out, workspace, stream);
}

}  // extern "C"
