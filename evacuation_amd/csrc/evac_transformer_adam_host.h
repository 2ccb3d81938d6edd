// Host side of the transformer leader's optimiser step, the part its two translation units share
// (evac_transformer_update_api.hip: one learner; evac_transformer_population_update_api.hip: a population): the trait TfAdam of
// evac_encoder_train_host.h's and evac_encoder_population_host.h's templates -- the encoder's 16 tensors per block in use behind
// the actor-critic's 13, what is refused of their sizes and of a population's strides, and the launch, whose kernel the unit
// names (k_adam_tf is defined in the one learner's unit alone, k_adam_tf_population in the population's): both take
// evac::TfAdamArgs.
#pragma once

#include "evac_transformer_adam_args.h"
#include "evac_transformer_train_host.h"

static_assert(evac::kTfAdamBlockTensors == evac::kTfgTensors && evac::kTfAdamMaxBlocks == evac::kTfgMaxBlocks,
              "k_adam_tf walks the tensors the gradient's kernels write");
static_assert(offsetof(evac_transformer_block_grads_t, norm2_b) == 15 * sizeof(float*) &&
                  sizeof(evac_transformer_grads_t) == evac::kTfAdamMaxBlocks * sizeof(evac_transformer_block_grads_t),
              "TfAdam::tensor walks a block as 16 consecutive pointers, wq first and norm2_b last");
static_assert(offsetof(evac_transformer_adam_state_t, header) == offsetof(evac_adam_state_t, header) &&
                  offsetof(evac_transformer_adam_state_t, exp_avg) == offsetof(evac_adam_state_t, exp_avg) &&
                  offsetof(evac_transformer_adam_state_t, exp_avg_sq) == offsetof(evac_adam_state_t, exp_avg_sq),
              "the state of the 13 tensors is evac_adam_state_t's");

namespace {

// One launch of the optimiser's kernel over `learners` learners: `kernel` is k_adam_tf (rest: nothing) or k_adam_tf_population
// (rest: its TfAdamStrides); the grid is every tensor's workgroups, times the learners.
template <class Kernel, class... Rest>
inline void tf_adam_launch(Kernel kernel, const evac::TfAdamArgs& q, unsigned learners, hipStream_t S, const Rest&... rest) {
    hipLaunchKernelGGL(kernel, dim3((unsigned)q.wg_end[q.nt - 1], learners), dim3(evac::kAdamBlock), 0, S, q, rest...);
}

// The transformer leader's side of the optimiser's templates.
struct TfAdam {
    using State = evac_transformer_adam_state_t;
    using Grads = evac_transformer_grads_t;
    using Args = evac::TfAdamArgs;
    using Strides = evac::TfAdamStrides;
    using EncoderStrides = evac_transformer_strides_t;
    struct Dims {
        int32_t dm, nb;
    };
    static Dims dims(const evac_transformer_t& T) { return {T.elem_dim, T.num_blocks}; }

    // its sizes as the gradient's entry looks at them: the blocks' number, the token width, the tokens
    static int check(int32_t D, const Dims& d) {
        if (d.nb < 1 || d.nb > kTransformerMaxBlocks) return EVAC_ERR_UNSUPPORTED;
        if (d.dm < 1 || d.dm > kTransformerMaxModelDim || D % d.dm != 0 || D / d.dm < 3) return EVAC_ERR_INVALID_ARGUMENT;
        if (D / d.dm > kTransformerMaxTokens) return EVAC_ERR_UNSUPPORTED;
        return EVAC_OK;
    }
    static Args fresh(const Dims& d) {
        Args q{};
        q.nt = evac::kAdamTensors + count(d);
        return q;
    }
    static int count(const Dims& d) { return evac::kTfAdamBlockTensors * d.nb; }                      // (blocks not in use: never looked at)
    static float* tensor(const Grads& g, int i) { return (&g.blocks[i / evac::kTfAdamBlockTensors].wq)[i % evac::kTfAdamBlockTensors]; }
    // evac_transformer_block_t: wq [3 dm][dm], bq [3 dm], wk, bk, wv, bv alike, dense_w [dm][3 dm], dense_b [dm], ff1_w [96][dm],
    // ff1_b [96], ff2_w [dm][96], ff2_b [dm], norm1_w, norm1_b, norm2_w, norm2_b [dm]
    static int size(int i, int32_t, const Dims& d) {
        const int H = kTransformerHeads, F = kTransformerFeedForward, dm = d.dm;
        const int n[evac::kTfAdamBlockTensors] = {H * dm * dm, H * dm, H * dm * dm, H * dm, H * dm * dm, H * dm, H * dm * dm, dm,
                                                  F * dm,      F,      F * dm,      dm,     dm,          dm,     dm,          dm};
        return n[i % evac::kTfAdamBlockTensors];
    }
    template <class Kernel, class... Rest>
    static void launch(Kernel kernel, const Args& q, unsigned learners, hipStream_t S, const Rest&... rest) {
        tf_adam_launch(kernel, q, learners, S, rest...);
    }

    // A population's strides of the tensors of the blocks in use -- parameters, gradients, moments -- held against the tensors
    // (transformer_strides_ok) and copied to where the gradient's kernels (`sq`) and the optimiser's (`aq`, behind the 13) read
    // them.  The strides of a block not in use stay 0: never looked at.
    static bool strides(const evac_transformer_t& T, int32_t, int32_t n_learners, const EncoderStrides* p, const EncoderStrides* g,
                        const EncoderStrides* m, evac::TfgLearnerStrides& sq, Strides& aq) {
        const int dm = T.elem_dim, nb = T.num_blocks;
        if (!transformer_strides_ok(p, dm, nb, n_learners) || !transformer_strides_ok(g, dm, nb, n_learners) ||
            !transformer_strides_ok(m, dm, nb, n_learners))
            return false;
        for (int b = 0; b < nb; ++b)
            for (int i = 0; i < evac::kTfgTensors; ++i) {
                const int t = evac::kAdamTensors + b * evac::kTfAdamBlockTensors + i;
                aq.p[t] = sq.p[b][i] = (&p->blocks[b].wq)[i];
                aq.g[t] = sq.g[b][i] = (&g->blocks[b].wq)[i];
                aq.m[t] = (&m->blocks[b].wq)[i];
            }
        return true;
    }
};

// evac_transformer_adam_step's checks and set-up with the encoder's sizes as the entry takes them.
inline int tf_adam_prepare(const evac_mlp_policy_grads_t* params, const evac_transformer_grads_t* enc_params,
                           const evac_mlp_policy_grads_t* grads, const evac_transformer_grads_t* enc_grads,
                           const evac_transformer_adam_state_t* state, const evac_adam_config_t* cfg, int32_t obs_dim, int32_t elem_dim,
                           int32_t num_blocks, evac::AdamArgs& o, evac::TfAdamArgs& q) {
    return encoder_adam_prepare<TfAdam>(params, enc_params, grads, enc_grads, state, cfg, obs_dim, TfAdam::Dims{elem_dim, num_blocks}, o, q);
}

}  // namespace
