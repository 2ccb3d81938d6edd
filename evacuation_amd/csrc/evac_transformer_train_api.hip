// Host side of the transformer leader's gradient (include/evac.h: evac_transformer_workspace_bytes,
// evac_transformer_minibatch_grad; kernels in evac_transformer_train.h and, launched as they are, evac_train.h's k_rpo_*<>; the
// linear network's checks and launches in evac_train_host.h, the encoder's in evac_transformer_host.h, the entry's body in
// evac_encoder_train_host.h around the trait TfGrad of evac_transformer_train_host.h): the encoder forwards, the
// three launches of evac_rpo_minibatch_grad on the encoded observations, dY, one launch per block backwards, the finish -- eight
// launches with two blocks and norm_adv.  No handle: errors come back through the return code alone and every refusal comes
// before the first HIP call.  No device allocation, no synchronisation: the call only enqueues work on the caller's stream.
#include <hip/hip_runtime.h>

#include <cstddef>
#include <cstdint>

#include "evac_transformer_train_host.h"

extern "C" {

int64_t evac_transformer_workspace_bytes(int32_t obs_dim, int64_t n_minibatch) {
    return encoder_workspace_bytes<TfGrad>(obs_dim, n_minibatch);
}

int evac_transformer_minibatch_grad(const evac_mlp_policy_t* policy, const evac_transformer_t* encoder, const evac_rpo_loss_config_t* cfg,
                                    int64_t batch_size, const float* b_obs, const float* b_actions, const float* b_logprobs,
                                    const float* b_advantages, const float* b_returns, const float* b_values, int64_t n_minibatch,
                                    const int64_t* mb_inds, const float* rpo_noise, uint64_t seed, uint64_t draw_counter,
                                    const evac_mlp_policy_grads_t* grads_out, const evac_transformer_grads_t* encoder_grads_out,
                                    float* stats_out, void* workspace, void* stream) {
    return encoder_minibatch_grad<TfGrad>(policy, encoder, cfg, batch_size, b_obs, b_actions, b_logprobs, b_advantages, b_returns,
                                          b_values, n_minibatch, mb_inds, rpo_noise, seed, draw_counter, grads_out, encoder_grads_out,
                                          stats_out, workspace, stream);
}

}  // extern "C"
