// Host side of the deep-sets leader's optimiser step and whole update (include/evac.h: evac_deepsets_adam_step,
// evac_deepsets_minibatch_step, evac_deepsets_update; k_adam_set in evac_deepsets_adam.h, the gradient's kernels in
// evac_deepsets_train.h and evac_train.h, plain for the step and gated by the optimiser's header for the update).  The checks are
// rpo_prepare's, SetGrad's and adam_prepare's (set_adam_prepare: evac_deepsets_adam_host.h, shared with the population's unit),
// the step's body is encoder_minibatch_grad's with the optimiser behind it, the walk over an update's steps is
// rpo_update_steps.  No handle: errors come back through the return code alone and every refusal comes before the first HIP
// call.  No device allocation, no synchronisation: every call only enqueues work on the caller's stream.
#include <hip/hip_runtime.h>

#include <cstddef>
#include <cstdint>

#include "evac_deepsets_adam.h"
#include "evac_deepsets_adam_host.h"

namespace {

void set_adam_launch(const evac::SetAdamArgs& q, hipStream_t S) {
    hipLaunchKernelGGL(evac::k_adam_set, dim3((unsigned)q.wg_end[evac::kSetAdamTensors - 1]), dim3(evac::kAdamBlock), 0, S, q);
}

}  // namespace

extern "C" {

int evac_deepsets_adam_step(const evac_mlp_policy_grads_t* params, const evac_deepsets_grads_t* enc_params,
                            const evac_mlp_policy_grads_t* grads, const evac_deepsets_grads_t* enc_grads,
                            const evac_deepsets_adam_state_t* state, const evac_adam_config_t* cfg, int32_t obs_dim, int32_t set_elem_dim,
                            const float* grad_sumsq, void* stream) {
    evac::AdamArgs o;
    evac::SetAdamArgs q;
    if (const int rc = set_adam_prepare(params, enc_params, grads, enc_grads, state, cfg, obs_dim, set_elem_dim, o, q); rc != EVAC_OK)
        return rc;
    if (!grad_sumsq) return EVAC_ERR_INVALID_ARGUMENT;
    q.sumsq = grad_sumsq;
    DeviceGuard g(device_of(state->header));
    set_adam_launch(q, (hipStream_t)stream);
    return hipGetLastError() == hipSuccess ? EVAC_OK : EVAC_ERR_HIP;
}

int evac_deepsets_minibatch_step(const evac_mlp_policy_t* policy, const evac_deepsets_t* encoder, const evac_rpo_loss_config_t* cfg,
                                 int64_t batch_size, const float* b_obs, const float* b_actions, const float* b_logprobs,
                                 const float* b_advantages, const float* b_returns, const float* b_values, int64_t n_minibatch,
                                 const int64_t* mb_inds, const float* rpo_noise, uint64_t seed, uint64_t draw_counter,
                                 const evac_mlp_policy_grads_t* grads_out, const evac_deepsets_grads_t* encoder_grads_out,
                                 float* stats_out, void* workspace, void* stream, const evac_mlp_policy_grads_t* params,
                                 const evac_deepsets_grads_t* enc_params, const evac_deepsets_adam_state_t* state,
                                 const evac_adam_config_t* adam_cfg) {
    evac::AdamArgs o;
    evac::SetAdamArgs q;
    return encoder_minibatch_grad<SetGrad>(
        policy, encoder, cfg, batch_size, b_obs, b_actions, b_logprobs, b_advantages, b_returns, b_values, n_minibatch, mb_inds, rpo_noise,
        seed, draw_counter, grads_out, encoder_grads_out, stats_out, workspace, stream,
        [&] {                                                                  // (behind the gradient's checks: policy and encoder are set)
            const int rc = set_adam_prepare(params, enc_params, grads_out, encoder_grads_out, state, adam_cfg, policy->obs_dim,
                                            encoder->set_elem_dim, o, q);
            if (rc == EVAC_OK) q.sumsq = stats_out + 7;
            return rc;
        },
        [&q](hipStream_t S) { set_adam_launch(q, S); });
}

int evac_deepsets_update(const evac_mlp_policy_t* policy, const evac_deepsets_t* encoder, const evac_mlp_policy_grads_t* params,
                         const evac_deepsets_grads_t* enc_params, const evac_mlp_policy_grads_t* grads,
                         const evac_deepsets_grads_t* enc_grads, const evac_rpo_loss_config_t* loss_cfg,
                         const evac_adam_config_t* adam_cfg, const evac_deepsets_adam_state_t* state, int64_t batch_size,
                         const float* b_obs, const float* b_actions, const float* b_logprobs, const float* b_advantages,
                         const float* b_returns, const float* b_values, int64_t n_minibatch, int32_t n_epochs, const int64_t* perms,
                         const float* rpo_noise, uint64_t seed, uint64_t first_draw_counter, int32_t use_target_kl, double target_kl,
                         float* stats_out, void* workspace, void* stream) {
    if (n_epochs < 1) return EVAC_ERR_INVALID_ARGUMENT;
    evac::RpoArgs a;
    evac::SetArgs s;
    if (const int rc = encoder_grad_prepare<SetGrad>(policy, encoder, loss_cfg, batch_size, b_obs, b_actions, b_logprobs, b_advantages,
                                                     b_returns, b_values, n_minibatch, perms, rpo_noise, seed, grads, enc_grads, stats_out,
                                                     workspace, a, s);
        rc != EVAC_OK)
        return rc;
    evac::AdamArgs o;
    evac::SetAdamArgs q;
    if (const int rc = set_adam_prepare(params, enc_params, grads, enc_grads, state, adam_cfg, policy->obs_dim, encoder->set_elem_dim, o, q);
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
                         const evac::RpoArgs inner = encoder_grad_step<SetGrad>(step, s);
                         encoder_adam_scalars(adam, q);
                         SetGrad::launch(inner, s, S, (const evac::AdamHeader*)adam.hdr);
                         set_adam_launch(q, S);
                     });
    return hipGetLastError() == hipSuccess ? EVAC_OK : EVAC_ERR_HIP;
}

}  // extern "C"
