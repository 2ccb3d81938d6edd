// Host side of the transformer leader's optimiser step, the part its two translation units share
// (evac_transformer_update_api.hip: one learner; evac_transformer_population_update_api.hip: a population): what
// evac_transformer_adam_step checks and sets up, and the launch, whose kernel the unit names (k_adam_tf is defined in the one
// learner's unit alone, k_adam_tf_population in the population's): both take evac::TfAdamArgs.
#pragma once

#include "evac_transformer_adam_args.h"
#include "evac_transformer_train_host.h"

static_assert(evac::kTfAdamBlockTensors == evac::kTfgTensors && evac::kTfAdamMaxBlocks == evac::kTfgMaxBlocks,
              "k_adam_tf walks the tensors the gradient's kernels write");

namespace {

inline float* const* block_tensors(const evac_transformer_block_grads_t& g) { return &g.wq; }
static_assert(offsetof(evac_transformer_block_grads_t, norm2_b) == 15 * sizeof(float*) &&
                  sizeof(evac_transformer_grads_t) == evac::kTfAdamMaxBlocks * sizeof(evac_transformer_block_grads_t),
              "block_tensors walks a block as 16 consecutive pointers, wq first and norm2_b last");
static_assert(offsetof(evac_transformer_adam_state_t, header) == offsetof(evac_adam_state_t, header) &&
                  offsetof(evac_transformer_adam_state_t, exp_avg) == offsetof(evac_adam_state_t, exp_avg) &&
                  offsetof(evac_transformer_adam_state_t, exp_avg_sq) == offsetof(evac_adam_state_t, exp_avg_sq),
              "the state of the 13 tensors is evac_adam_state_t's");

// What evac_transformer_adam_step checks and sets up: adam_prepare for the 13 tensors (into `o`), then the encoder's 16 per block
// in use -- its sizes before its pointers, as the gradient's entry looks at them.
inline int tf_adam_prepare(const evac_mlp_policy_grads_t* params, const evac_transformer_grads_t* enc_params,
                           const evac_mlp_policy_grads_t* grads, const evac_transformer_grads_t* enc_grads,
                           const evac_transformer_adam_state_t* state, const evac_adam_config_t* cfg, int32_t obs_dim, int32_t elem_dim,
                           int32_t num_blocks, evac::AdamArgs& o, evac::TfAdamArgs& q) {
    if (!state || !enc_params || !enc_grads) return EVAC_ERR_INVALID_ARGUMENT;
    const evac_adam_state_t linear{state->header, state->exp_avg, state->exp_avg_sq};
    if (const int rc = adam_prepare(params, grads, &linear, cfg, obs_dim, o); rc != EVAC_OK) return rc;
    if (num_blocks < 1 || num_blocks > kTransformerMaxBlocks) return EVAC_ERR_UNSUPPORTED;
    const int dm = elem_dim, D = obs_dim;
    if (dm < 1 || dm > kTransformerMaxModelDim || D % dm != 0 || D / dm < 3) return EVAC_ERR_INVALID_ARGUMENT;
    if (D / dm > kTransformerMaxTokens) return EVAC_ERR_UNSUPPORTED;
    q = evac::TfAdamArgs{};
    const evac_transformer_grads_t* sets[4] = {enc_params, enc_grads, &state->enc_exp_avg, &state->enc_exp_avg_sq};
    float* const* lin[4] = {o.p, o.g, o.m, o.v};
    float** dst[4] = {q.p, q.g, q.m, q.v};
    for (int k = 0; k < 4; ++k) {
        for (int i = 0; i < evac::kAdamTensors; ++i) dst[k][i] = lin[k][i];
        for (int b = 0; b < num_blocks; ++b) {                                 // (blocks not in use: never looked at)
            if (!transformer_block_all_set(sets[k]->blocks[b])) return EVAC_ERR_INVALID_ARGUMENT;
            for (int i = 0; i < evac::kTfAdamBlockTensors; ++i)
                dst[k][evac::kAdamTensors + b * evac::kTfAdamBlockTensors + i] = block_tensors(sets[k]->blocks[b])[i];
        }
    }
    // evac_transformer_block_t: wq [3 dm][dm], bq [3 dm], wk, bk, wv, bv alike, dense_w [dm][3 dm], dense_b [dm], ff1_w [96][dm],
    // ff1_b [96], ff2_w [dm][96], ff2_b [dm], norm1_w, norm1_b, norm2_w, norm2_b [dm]
    const int H = kTransformerHeads, F = kTransformerFeedForward;
    const int blk_n[evac::kTfAdamBlockTensors] = {H * dm * dm, H * dm, H * dm * dm, H * dm, H * dm * dm, H * dm, H * dm * dm, dm,
                                                  F * dm,      F,      F * dm,      dm,     dm,          dm,     dm,          dm};
    q.nt = evac::kAdamTensors + evac::kTfAdamBlockTensors * num_blocks;
    int wgs = 0;
    for (int i = 0; i < q.nt; ++i) {
        q.n[i] = i < evac::kAdamTensors ? o.end[i] - (i ? o.end[i - 1] : 0) : blk_n[(i - evac::kAdamTensors) % evac::kTfAdamBlockTensors];
        q.wg_end[i] = (wgs += (q.n[i] + evac::kAdamBlock - 1) / evac::kAdamBlock);
    }
    encoder_adam_scalars(o, q);
    return EVAC_OK;
}
// One launch of the optimiser's kernel over `learners` learners: `kernel` is k_adam_tf (rest: nothing) or k_adam_tf_population
// (rest: its TfAdamStrides); the grid is every tensor's workgroups, times the learners.
template <class Kernel, class... Rest>
inline void tf_adam_launch(Kernel kernel, const evac::TfAdamArgs& q, unsigned learners, hipStream_t S, const Rest&... rest) {
    hipLaunchKernelGGL(kernel, dim3((unsigned)q.wg_end[q.nt - 1], learners), dim3(evac::kAdamBlock), 0, S, q, rest...);
}

}  // namespace
