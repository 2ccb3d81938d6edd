// Device code of libevac: the argument struct of the deep-sets leader's optimiser step, apart from its kernel (k_adam_set,
// evac_deepsets_adam.h) so that the population's unit (evac_deepsets_population.h: k_adam_set_population) takes the same struct
// without defining that kernel a second time.  No kernel is defined here.
#pragma once

#include "evac_train.h"

namespace evac {

constexpr int kSetAdamTensors = kAdamTensors + 6;   // evac_mlp_policy_grads_t, then evac_deepsets_grads_t
struct SetAdamArgs {
    float *p[kSetAdamTensors], *g[kSetAdamTensors], *m[kSetAdamTensors], *v[kSetAdamTensors];
    int wg_end[kSetAdamTensors];                // running workgroup counts: tensor i has workgroups [wg_end[i - 1], wg_end[i])
    int n[kSetAdamTensors];                     // elements of tensor i
    AdamHeader* hdr;
    const float* sumsq;                         // the sum of squares of all gradient entries, 19 tensors (device)
    const float* stats;                         // the step's statistics (approx_kl at [5]) for the early exit, or NULL
    double lr, beta1, beta2, target_kl;
    float max_norm, w, b2, u, eps;              // as AdamArgs'
    int gated, epoch_last, use_target_kl;
};
static_assert(sizeof(SetAdamArgs) <= 1024, "k_adam_set's kernel arguments");

// ... and what k_adam_set_population takes behind it: the learners' strides (the host fills them in evac_deepsets_adam_host.h)
struct SetAdamStrides {
    int64_t p[kSetAdamTensors], g[kSetAdamTensors], m[kSetAdamTensors];   // floats: parameters, gradients, moments (both of them)
    int64_t hdr;                                // bytes
    int64_t stats;                              // floats of stats_out per learner
};

}  // namespace evac
