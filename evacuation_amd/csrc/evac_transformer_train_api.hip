// Host side of the transformer leader's gradient (include/evac.h: evac_transformer_workspace_bytes,
// evac_transformer_minibatch_grad; kernels in evac_transformer_train.h and, launched as they are, evac_train.h's k_rpo_*<>; the
// linear network's checks and launches in evac_train_host.h, the encoder's in evac_transformer_host.h, the entry's body in
// evac_encoder_train_host.h around the trait TfGrad below): the encoder forwards, the
// three launches of evac_rpo_minibatch_grad on the encoded observations, dY, one launch per block backwards, the finish -- eight
// launches with two blocks and norm_adv.  No handle: errors come back through the return code alone and every refusal comes
// before the first HIP call.  No device allocation, no synchronisation: the call only enqueues work on the caller's stream.
#include <hip/hip_runtime.h>

#include <cstddef>
#include <cstdint>
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
static_assert(sizeof(evac::TfgArgs) + 8 <= 4096, "k_tf_backward: arguments beyond the kernel-argument segment");

namespace {

// The transformer leader's side of evac_encoder_train_host.h's templates.
struct TfGrad {
    using Encoder = evac_transformer_t;
    using Grads = evac_transformer_grads_t;
    using Args = evac::TfgArgs;

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

    // The launches of one minibatch's gradient, all 13 + 16 num_blocks tensors.
    static void launch(const evac::RpoArgs& a, const Args& s, hipStream_t S) {
        const int64_t M = s.M;
        const int64_t enc_wgs = (M + evac::kTfgEncodeWaves - 1) / evac::kTfgEncodeWaves;
        hipLaunchKernelGGL(evac::k_tf_encode, dim3((unsigned)(enc_wgs > evac::kTfgEncodeMaxWgs ? evac::kTfgEncodeMaxWgs : enc_wgs)),
                           dim3(evac::kTfgEncodeBlock), 0, S, s);
        rpo_launch(a, S);
        const int64_t tiles = (M + evac::kTfgTile - 1) / evac::kTfgTile;
        hipLaunchKernelGGL(evac::k_tf_dy, dim3((unsigned)(tiles > 65536 ? 65536 : tiles)), dim3(evac::kTfgEncodeBlock), 0, S, s);
        for (int b = s.nb - 1; b >= 0; --b)
            hipLaunchKernelGGL(evac::k_tf_backward, dim3((unsigned)s.P), dim3(evac::kTfgBlock), 0, S, s, b);
        hipLaunchKernelGGL(evac::k_tf_finish, dim3((unsigned)(s.nb * evac::kTfgFinishWgs)), dim3(evac::kTfgEncodeBlock), 0, S, s);
    }
};

}  // namespace

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
