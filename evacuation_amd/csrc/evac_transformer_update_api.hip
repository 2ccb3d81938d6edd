// Host side of the transformer leader's optimiser step and whole update (include/evac.h: evac_transformer_adam_step,
// evac_transformer_minibatch_step, evac_transformer_update; k_adam_tf in evac_transformer_adam.h, its checks and launch in
// evac_transformer_adam_host.h, which the population's unit shares; the gradient's kernels in
// evac_transformer_train.h and evac_train.h, plain for the step and gated by the optimiser's header for the update).  The checks
// are rpo_prepare's, TfGrad's and adam_prepare's, the step's body is encoder_minibatch_grad's with the optimiser behind it, the
// walk over an update's steps is rpo_update_steps: evac_deepsets_update_api.hip with another trait.  No handle: errors come back
// through the return code alone and every refusal comes before the first HIP call.  No device allocation, no synchronisation:
// every call only enqueues work on the caller's stream.
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
    evac::AdamArgs o;
    evac::TfAdamArgs q;
    if (const int rc = tf_adam_prepare(params, enc_params, grads, enc_grads, state, cfg, obs_dim, elem_dim, num_blocks, o, q); rc != EVAC_OK)
        return rc;
    if (!grad_sumsq) return EVAC_ERR_INVALID_ARGUMENT;
    q.sumsq = grad_sumsq;
    DeviceGuard g(device_of(state->header));
    tf_adam_launch(evac::k_adam_tf, q, 1u, (hipStream_t)stream);
    return hipGetLastError() == hipSuccess ? EVAC_OK : EVAC_ERR_HIP;
}

int evac_transformer_minibatch_step(const evac_mlp_policy_t* policy, const evac_transformer_t* encoder, const evac_rpo_loss_config_t* cfg,
                                    int64_t batch_size, const float* b_obs, const float* b_actions, const float* b_logprobs,
                                    const float* b_advantages, const float* b_returns, const float* b_values, int64_t n_minibatch,
                                    const int64_t* mb_inds, const float* rpo_noise, uint64_t seed, uint64_t draw_counter,
                                    const evac_mlp_policy_grads_t* grads_out, const evac_transformer_grads_t* encoder_grads_out,
                                    float* stats_out, void* workspace, void* stream, const evac_mlp_policy_grads_t* params,
                                    const evac_transformer_grads_t* enc_params, const evac_transformer_adam_state_t* state,
                                    const evac_adam_config_t* adam_cfg) {
    evac::AdamArgs o;
    evac::TfAdamArgs q;
    return encoder_minibatch_grad<TfGrad>(
        policy, encoder, cfg, batch_size, b_obs, b_actions, b_logprobs, b_advantages, b_returns, b_values, n_minibatch, mb_inds, rpo_noise,
        seed, draw_counter, grads_out, encoder_grads_out, stats_out, workspace, stream,
        [&] {                                                                  // (behind the gradient's checks: policy and encoder are set)
            const int rc = tf_adam_prepare(params, enc_params, grads_out, encoder_grads_out, state, adam_cfg, policy->obs_dim,
                                           encoder->elem_dim, encoder->num_blocks, o, q);
            if (rc == EVAC_OK) q.sumsq = stats_out + 7;
            return rc;
        },
        [&q](hipStream_t S) { tf_adam_launch(evac::k_adam_tf, q, 1u, S); });
}

int evac_transformer_update(const evac_mlp_policy_t* policy, const evac_transformer_t* encoder, const evac_mlp_policy_grads_t* params,
                            const evac_transformer_grads_t* enc_params, const evac_mlp_policy_grads_t* grads,
                            const evac_transformer_grads_t* enc_grads, const evac_rpo_loss_config_t* loss_cfg,
                            const evac_adam_config_t* adam_cfg, const evac_transformer_adam_state_t* state, int64_t batch_size,
                            const float* b_obs, const float* b_actions, const float* b_logprobs, const float* b_advantages,
                            const float* b_returns, const float* b_values, int64_t n_minibatch, int32_t n_epochs, const int64_t* perms,
                            const float* rpo_noise, uint64_t seed, uint64_t first_draw_counter, int32_t use_target_kl, double target_kl,
                            float* stats_out, void* workspace, void* stream) {
    if (n_epochs < 1) return EVAC_ERR_INVALID_ARGUMENT;
    evac::RpoArgs a;
    evac::TfgArgs s;
    if (const int rc = encoder_grad_prepare<TfGrad>(policy, encoder, loss_cfg, batch_size, b_obs, b_actions, b_logprobs, b_advantages,
                                                    b_returns, b_values, n_minibatch, perms, rpo_noise, seed, grads, enc_grads, stats_out,
                                                    workspace, a, s);
        rc != EVAC_OK)
        return rc;
    evac::AdamArgs o;
    evac::TfAdamArgs q;
    if (const int rc = tf_adam_prepare(params, enc_params, grads, enc_grads, state, adam_cfg, policy->obs_dim, encoder->elem_dim,
                                       encoder->num_blocks, o, q);
        rc != EVAC_OK)
        return rc;
    o.gated = 1;
    o.use_target_kl = use_target_kl != 0;
    o.target_kl = target_kl;
    const int dev = device_of(workspace);
    DeviceGuard g(dev);
    if (rpo_raise_lds<evac::k_rpo_grad<const evac::AdamHeader*>>(a.D, dev) != EVAC_OK) return EVAC_ERR_HIP;
    hipStream_t S = (hipStream_t)stream;
    // stop, steps_run, epochs_run (and the ticket, zero anyway)
    if (hipMemsetAsync((char*)state->header + offsetof(evac::AdamHeader, stop), 0, 16, S) != hipSuccess) {
        (void)hipGetLastError();
        return EVAC_ERR_HIP;
    }
    rpo_update_steps(a, o, batch_size, n_minibatch, n_epochs, perms, rpo_noise, stats_out, first_draw_counter,
                     [&s, &q, S](const evac::RpoArgs& step, const evac::AdamArgs& adam, uint64_t) {
                         const evac::RpoArgs inner = encoder_grad_step<TfGrad>(step, s);
                         encoder_adam_scalars(adam, q);
                         TfGrad::launch(inner, s, S, (const evac::AdamHeader*)adam.hdr);
                         tf_adam_launch(evac::k_adam_tf, q, 1u, S);
                     });
    return hipGetLastError() == hipSuccess ? EVAC_OK : EVAC_ERR_HIP;
}

}  // extern "C"
