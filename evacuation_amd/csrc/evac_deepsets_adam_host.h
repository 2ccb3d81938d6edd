// Host side of the deep-sets leader's optimiser step, the part its two translation units share (evac_deepsets_update_api.hip:
// one learner; evac_deepsets_population_api.hip: a population): what evac_deepsets_adam_step checks and sets up.  The kernels
// stay in the units (k_adam_set, k_adam_set_population): both take evac::SetAdamArgs.
#pragma once

#include "evac_deepsets_adam_args.h"
#include "evac_deepsets_train_host.h"

namespace {

inline float* const* set_tensors(const evac_deepsets_grads_t& g) { return &g.phi_w1; }
static_assert(sizeof(evac_deepsets_grads_t) == 6 * sizeof(float*) && offsetof(evac_deepsets_grads_t, rho_b) == 5 * sizeof(float*),
              "set_tensors walks the struct as 6 consecutive pointers, phi_w1 first and rho_b last");
static_assert(offsetof(evac_deepsets_adam_state_t, exp_avg) == offsetof(evac_adam_state_t, exp_avg) &&
                  offsetof(evac_deepsets_adam_state_t, exp_avg_sq) == offsetof(evac_adam_state_t, exp_avg_sq),
              "the state of the 13 tensors is evac_adam_state_t's");

// What evac_deepsets_adam_step checks and sets up: adam_prepare for the 13 tensors (into `o`), then the encoder's six.
inline int set_adam_prepare(const evac_mlp_policy_grads_t* params, const evac_deepsets_grads_t* enc_params,
                            const evac_mlp_policy_grads_t* grads, const evac_deepsets_grads_t* enc_grads,
                            const evac_deepsets_adam_state_t* state, const evac_adam_config_t* cfg, int32_t obs_dim, int32_t set_elem_dim,
                            evac::AdamArgs& o, evac::SetAdamArgs& q) {
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
}  // namespace
