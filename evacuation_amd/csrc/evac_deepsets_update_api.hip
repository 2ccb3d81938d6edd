// Host side of the deep-sets leader's optimiser step and whole update (include/evac.h: evac_deepsets_adam_step,
// evac_deepsets_minibatch_step, evac_deepsets_update; k_adam_set in evac_deepsets_adam.h, the gradient's kernels in
// evac_deepsets_train.h and evac_train.h, plain for the step and gated by the optimiser's header for the update).  The checks are
// rpo_prepare's, SetGrad's and adam_prepare's, the step's body is encoder_minibatch_grad's with the optimiser behind it, the walk
// over an update's steps is rpo_update_steps.  No handle: errors
// come back through the return code alone and every refusal comes before the first HIP call.  No device allocation, no
// synchronisation: every call only enqueues work on the caller's stream.
#include <hip/hip_runtime.h>

#include <cstddef>
#include <cstdint>

#include "evac_deepsets_adam.h"
#include "evac_deepsets_train_host.h"

namespace {

inline float* const* set_tensors(const evac_deepsets_grads_t& g) { return &g.phi_w1; }
static_assert(sizeof(evac_deepsets_grads_t) == 6 * sizeof(float*) && offsetof(evac_deepsets_grads_t, rho_b) == 5 * sizeof(float*),
              "set_tensors walks the struct as 6 consecutive pointers, phi_w1 first and rho_b last");
static_assert(offsetof(evac_deepsets_adam_state_t, exp_avg) == offsetof(evac_adam_state_t, exp_avg) &&
                  offsetof(evac_deepsets_adam_state_t, exp_avg_sq) == offsetof(evac_adam_state_t, exp_avg_sq),
              "the state of the 13 tensors is evac_adam_state_t's");

// What evac_deepsets_adam_step checks and sets up: adam_prepare for the 13 tensors (into `o`), then the encoder's six.
int set_adam_prepare(const evac_mlp_policy_grads_t* params, const evac_deepsets_grads_t* enc_params, const evac_mlp_policy_grads_t* grads,
                     const evac_deepsets_grads_t* enc_grads, const evac_deepsets_adam_state_t* state, const evac_adam_config_t* cfg,
                     int32_t obs_dim, int32_t set_elem_dim, evac::AdamArgs& o, evac::SetAdamArgs& q) {
    if (!state || !enc_params || !enc_grads) return EVAC_ERR_INVALID_ARGUMENT;
    const evac_adam_state_t linear{state->header, state->exp_avg, state->exp_avg_sq};
    if (const int rc = adam_prepare(params, grads, &linear, cfg, obs_dim, o); rc != EVAC_OK) return rc;
    const int ed = set_elem_dim;
    if (ed < 1 || ed > evac::kSetTrainMaxElemDim || obs_dim % ed != 0 || obs_dim / ed < 3) return EVAC_ERR_INVALID_ARGUMENT;
    q = evac::SetAdamArgs{};
    const evac_deepsets_grads_t* sets[4] = {enc_params, enc_grads, &state->enc_exp_avg, &state->enc_exp_avg_sq};
    float* const* lin[4] = {o.p, o.g, o.m, o.v};
    float** dst[4] = {q.p, q.g, q.m, q.v};
    for (int k = 0; k < 4; ++k) {
        for (int i = 0; i < evac::kAdamTensors; ++i) dst[k][i] = lin[k][i];
        for (int i = 0; i < 6; ++i) {
            if (!set_tensors(*sets[k])[i]) return EVAC_ERR_INVALID_ARGUMENT;
            dst[k][evac::kAdamTensors + i] = set_tensors(*sets[k])[i];
        }
    }
    // evac_deepsets_t: phi_w1 [24][ed], phi_b1 [24], phi_w2 [24][24], phi_b2 [24], rho_w [D][24], rho_b [D]
    const int H = evac::kSetTrainHidden, D = obs_dim;
    const int enc_n[6] = {H * ed, H, H * H, H, D * H, D};
    int wgs = 0;
    for (int i = 0; i < evac::kSetAdamTensors; ++i) {
        q.n[i] = i < evac::kAdamTensors ? o.end[i] - (i ? o.end[i - 1] : 0) : enc_n[i - evac::kAdamTensors];
        q.wg_end[i] = (wgs += (q.n[i] + evac::kAdamBlock - 1) / evac::kAdamBlock);
    }
    encoder_adam_scalars(o, q);
    return EVAC_OK;
}
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
