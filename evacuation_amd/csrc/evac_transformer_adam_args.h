// Device code of libevac: the argument struct of the transformer leader's optimiser step, apart from its kernel (k_adam_tf,
// evac_transformer_adam.h) so that the population's unit (evac_transformer_population_train.h: k_adam_tf_population) takes the
// same struct without defining that kernel a second time.  No kernel is defined here.
#pragma once

#include "evac_train.h"

namespace evac {

constexpr int kTfAdamBlockTensors = 16;                                    // evac_transformer_block_grads_t
constexpr int kTfAdamMaxBlocks = 2;
constexpr int kTfAdamTensors = kAdamTensors + kTfAdamBlockTensors * kTfAdamMaxBlocks;   // 45
struct TfAdamArgs {
    float *p[kTfAdamTensors], *g[kTfAdamTensors], *m[kTfAdamTensors], *v[kTfAdamTensors];
    int wg_end[kTfAdamTensors];                 // running workgroup counts: tensor i has workgroups [wg_end[i - 1], wg_end[i])
    int n[kTfAdamTensors];                      // elements of tensor i
    AdamHeader* hdr;
    const float* sumsq;                         // the sum of squares of all gradient entries, nt tensors (device)
    const float* stats;                         // the step's statistics (approx_kl at [5]) for the early exit, or NULL
    double lr, beta1, beta2, target_kl;
    float max_norm, w, b2, u, eps;              // as AdamArgs'
    int gated, epoch_last, use_target_kl;
    int nt;                                     // tensors in use: 13 + 16 num_blocks
};
static_assert(sizeof(TfAdamArgs) <= 4096, "k_adam_tf's kernel arguments: the kernel-argument segment holds 4 KB");

// ... and what k_adam_tf_population takes behind it: the learners' strides (the host fills them in evac_transformer_adam_host.h)
struct TfAdamStrides {
    int64_t p[kTfAdamTensors], g[kTfAdamTensors], m[kTfAdamTensors];   // floats: parameters, gradients, moments (both of them)
    int64_t hdr;                                // bytes
    int64_t stats;                              // floats of stats_out per learner
};

}  // namespace evac
