// Host side of the transformer leader's training entries, the part its translation units share
// (evac_transformer_train_api.hip: the gradient; evac_transformer_update_api.hip: the gradient with the optimiser, and the whole
// update; evac_transformer_population_update_api.hip: a population's update): the workspace's layout, what the entries check of
// the encoder, its fields of the kernels' argument struct and the encoder's launches in front of and behind the actor-critic's,
// as the trait TfGrad of evac_encoder_train_host.h's templates.
#pragma once

#include <string>

#include "evac_transformer_train.h"
#include "evac_encoder_train_host.h"
#include "evac_transformer_host.h"

static_assert(evac::kTfgHeads == kTransformerHeads && evac::kTfgFeedForward == kTransformerFeedForward &&
                  evac::kTfgDm == kTransformerMaxModelDim && evac::kTfgMaxBlocks == kTransformerMaxBlocks &&
                  evac::kTfgLnEps == kTransformerLnEps && kTransformerMaxTokens == 64,
              "evac_transformer_host.h's limits are the gradient kernels'");
static_assert(sizeof(evac_transformer_block_t) == evac::kTfgTensors * sizeof(void*) &&
                  sizeof(evac_transformer_block_grads_t) == evac::kTfgTensors * sizeof(void*),
              "evac_transformer_block_t / evac_transformer_block_grads_t: the 16 pointers TfgBlock copies in order");
static_assert(sizeof(evac::TfgArgs) + 8 + sizeof(void*) <= 4096, "k_tf_backward: arguments beyond the kernel-argument segment");

namespace {

// The transformer leader's side of evac_encoder_train_host.h's templates.
struct TfGrad {
    using Encoder = evac_transformer_t;
    using Grads = evac_transformer_grads_t;
    using Args = evac::TfgArgs;
    using LearnerStrides = evac::TfgLearnerStrides;       // (a population's: behind the gate in `tail`)

    // The workspace: evac_rpo_minibatch_grad's own (for a batch of M rows of D floats) | the ticket and the slots | Y | dX | X1 |
    // the gathered actions, log-probabilities, advantages, returns, values | the index vector | the partials of two blocks; every
    // part on a 256-byte boundary.
    struct Layout {
        int64_t header, Y, dX, X1;
        GatheredLayout cols;
        int64_t parts, total;
    };
    static Layout layout(int32_t D, int64_t M) {
        Layout L;
        WsCursor c = encoder_ws_cursor(D, M);
        const int64_t f = (int64_t)sizeof(float);
        L.header = c.take(evac::kTfgHeaderBytes);
        L.Y = c.take(M * D * f);
        L.dX = c.take(M * D * f);
        L.X1 = c.take(M * D * f);
        L.cols = take_gathered(c, M);
        L.parts = c.take((int64_t)evac::kTfgMaxBlocks * evac::tfg_parts(M) * evac::kTfgPart * f);
        L.total = c.o;
        return L;
    }

    // What evac_transformer_minibatch_grad checks of the encoder behind rpo_prepare's checks -- its sizes before its pointers --
    // and the encoder's fields of TfgArgs.
    static int check(const Encoder& T, const Grads& G, int D, Args& s) {
        std::string why;
        if (const int rc = transformer_check_sizes(T, why); rc != EVAC_OK) return rc;
        const int dm = T.elem_dim;
        if (dm < 1 || dm > kTransformerMaxModelDim || D % dm != 0 || D / dm < 3) return EVAC_ERR_INVALID_ARGUMENT;   // (N + 2 tokens, N >= 1)
        if (D / dm > kTransformerMaxTokens) return EVAC_ERR_UNSUPPORTED;                                             // (one wave holds them)
        if (const int rc = transformer_check_blocks(T, why); rc != EVAC_OK) return rc;
        for (int b = 0; b < T.num_blocks; ++b)
            if (!transformer_block_all_set(G.blocks[b])) return EVAC_ERR_INVALID_ARGUMENT;
        s = Args{};
        for (int b = 0; b < T.num_blocks; ++b) {
            const float* const* w = &T.blocks[b].wq;                   // (16 pointers in order: asserted above)
            float* const* g = &G.blocks[b].wq;
            for (int i = 0; i < evac::kTfgTensors; ++i) {
                s.blk[b].w[i] = w[i];
                s.blk[b].g[i] = g[i];
            }
        }
        s.D = D; s.dm = dm; s.S = D / dm; s.nb = T.num_blocks; s.resid = T.use_resid != 0;
        return EVAC_OK;
    }
    // The encoder's own parts of the workspace and the fields that depend on the minibatch's size.
    static void shape(Args& s, const Layout& L, char* ws, int64_t M) {
        s.dX = (float*)(ws + L.dX); s.X1 = (float*)(ws + L.X1);
        const int p0 = evac::tfg_parts(M);
        s.chunk = (int)((M + p0 - 1) / p0);
        s.P = (int)((M + s.chunk - 1) / s.chunk);                                 // (P <= p0: the workspace's bound)
    }

    // The encoder's launches of one minibatch's gradient, in front of the actor-critic's (the encoder forwards) and behind them
    // (dY, one launch per block backwards, the finish): a grid of `y` rows, one per learner; `tail` is what the kernels take
    // behind `s`.
    template <class... Tail>
    static void encode(const Args& s, unsigned y, hipStream_t S, Tail... tail) {
        const int64_t enc_wgs = (s.M + evac::kTfgEncodeWaves - 1) / evac::kTfgEncodeWaves;
        hipLaunchKernelGGL(evac::k_tf_encode<Tail...>, dim3((unsigned)(enc_wgs > evac::kTfgEncodeMaxWgs ? evac::kTfgEncodeMaxWgs : enc_wgs), y),
                           dim3(evac::kTfgEncodeBlock), 0, S, s, tail...);
    }
    template <class... Tail>
    static void backward(const Args& s, unsigned y, hipStream_t S, Tail... tail) {
        const int64_t tiles = (s.M + evac::kTfgTile - 1) / evac::kTfgTile;
        hipLaunchKernelGGL(evac::k_tf_dy<Tail...>, dim3((unsigned)(tiles > 65536 ? 65536 : tiles), y), dim3(evac::kTfgEncodeBlock), 0, S, s,
                           tail...);
        for (int b = s.nb - 1; b >= 0; --b)
            hipLaunchKernelGGL(evac::k_tf_backward<Tail...>, dim3((unsigned)s.P, y), dim3(evac::kTfgBlock), 0, S, s, b, tail...);
        hipLaunchKernelGGL(evac::k_tf_finish<Tail...>, dim3((unsigned)(s.nb * evac::kTfgFinishWgs), y), dim3(evac::kTfgEncodeBlock), 0, S, s,
                           tail...);
    }
};

}  // namespace
