// Host side of the transformer leader's optimiser step and whole update (include/evac.h: evac_transformer_adam_step,
// evac_transformer_minibatch_step, evac_transformer_update; k_adam_tf in evac_transformer_adam.h, the gradient's kernels in
// evac_transformer_train.h and evac_train.h, plain for the step and gated by the optimiser's header for the update).  The unit
// names its kernel and traits (TfGrad, TfAdam); the bodies are evac_encoder_train_host.h's.  No handle: errors come back through
// the return code alone and every refusal comes before the first HIP call.  No device allocation, no synchronisation: every call
// only enqueues work on the caller's stream.
#include <hip/hip_runtime.h>

#include <cstddef>
#include <cstdint>

#include "evac_transformer_adam.h"
#include "evac_transformer_adam_host.h"

extern "C" {

int evac_transformer_adam_step(const evac_mlp_policy_grads_t* params, const evac_transformer_grads_t* enc_params,
                               const evac_mlp_policy_grads_t* grads, const evac_transformer_grads_t* enc_grads,
                               const evac_transformer_adam_state_t* state, const evac_adam_config_t* cfg, int32_t obs_dim,
                               int32_t elem_dim, int32_t num_blocks, const float* grad_sumsq, void* stream) {
    return encoder_adam_step<TfAdam>(evac::k_adam_tf, params, enc_params, grads, enc_grads, state, cfg, obs_dim,
                                     TfAdam::Dims{elem_dim, num_blocks}, grad_sumsq, stream);
}

int evac_transformer_minibatch_step(const evac_mlp_policy_t* policy, const evac_transformer_t* encoder, const evac_rpo_loss_config_t* cfg,
                                    int64_t batch_size, const float* b_obs, const float* b_actions, const float* b_logprobs,
                                    const float* b_advantages, const float* b_returns, const float* b_values, int64_t n_minibatch,
                                    const int64_t* mb_inds, const float* rpo_noise, uint64_t seed, uint64_t draw_counter,
                                    const evac_mlp_policy_grads_t* grads_out, const evac_transformer_grads_t* encoder_grads_out,
                                    float* stats_out, void* workspace, void* stream, const evac_mlp_policy_grads_t* params,
                                    const evac_transformer_grads_t* enc_params, const evac_transformer_adam_state_t* state,
                                    const evac_adam_config_t* adam_cfg) {
    return encoder_minibatch_step<TfGrad, TfAdam>(evac::k_adam_tf, policy, encoder, cfg, batch_size, b_obs, b_actions, b_logprobs,
                                                  b_advantages, b_returns, b_values, n_minibatch, mb_inds, rpo_noise, seed, draw_counter,
                                                  grads_out, encoder_grads_out, stats_out, workspace, stream, params, enc_params, state,
                                                  adam_cfg);
}

int evac_transformer_update(const evac_mlp_policy_t* policy, const evac_transformer_t* encoder, const evac_mlp_policy_grads_t* params,
                            const evac_transformer_grads_t* enc_params, const evac_mlp_policy_grads_t* grads,
                            const evac_transformer_grads_t* enc_grads, const evac_rpo_loss_config_t* loss_cfg,
                            const evac_adam_config_t* adam_cfg, const evac_transformer_adam_state_t* state, int64_t batch_size,
                            const float* b_obs, const float* b_actions, const float* b_logprobs, const float* b_advantages,
                            const float* b_returns, const float* b_values, int64_t n_minibatch, int32_t n_epochs, const int64_t* perms,
                            const float* rpo_noise, uint64_t seed, uint64_t first_draw_counter, int32_t use_target_kl, double target_kl,
                            float* stats_out, void* workspace, void* stream) {
    return encoder_update<TfGrad, TfAdam>(evac::k_adam_tf, policy, encoder, params, enc_params, grads, enc_grads, loss_cfg, adam_cfg, state,
                                          batch_size, b_obs, b_actions, b_logprobs, b_advantages, b_returns, b_values, n_minibatch,
                                          n_epochs, perms, rpo_noise, seed, first_draw_counter, use_target_kl, target_kl, stats_out,
                                          workspace, stream);
}

}  // extern "C"
