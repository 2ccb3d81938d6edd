// Host side of the transformer leader's gradient (include/evac.h: evac_transformer_workspace_bytes,
// evac_transformer_minibatch_grad; kernels in evac_transformer_train.h and, launched as they are, evac_train.h's k_rpo_*<>; the
// linear network's checks and launches in evac_train_host.h, the encoder's in evac_transformer_host.h): the encoder forwards, the
// three launches of evac_rpo_minibatch_grad on the encoded observations, dY, one launch per block backwards, the finish -- eight
// launches with two blocks and norm_adv.  No handle: errors come back through the return code alone and every refusal comes
// before the first HIP call.  No device allocation, no synchronisation: the call only enqueues work on the caller's stream.
#include <hip/hip_runtime.h>

#include <cstddef>
#include <cstdint>
#include <string>

#include "evac_transformer_train.h"
#include "evac_train_host.h"
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

constexpr int64_t kTfgAlign = 256;
inline int64_t tfg_round_up(int64_t n) { return (n + kTfgAlign - 1) / kTfgAlign * kTfgAlign; }

// The workspace: evac_rpo_minibatch_grad's own (for a batch of M rows of D floats) | the ticket and the slots | Y | dX | X1 | the
// gathered actions, log-probabilities, advantages, returns, values | the index vector | the partials of two blocks; every part
// on a 256-byte boundary.
struct TfgLayout {
    int64_t header, Y, dX, X1, act, lp, adv, ret, val, ident, parts, total;
};
inline TfgLayout tfg_layout(int32_t D, int64_t M) {
    TfgLayout L;
    int64_t o = tfg_round_up(evac_rpo_workspace_bytes(D, M));
    const auto take = [&o](int64_t bytes) {
        const int64_t at = o;
        o += tfg_round_up(bytes);
        return at;
    };
    const int64_t f = (int64_t)sizeof(float);
    L.header = take(evac::kTfgHeaderBytes);
    L.Y = take(M * D * f);
    L.dX = take(M * D * f);
    L.X1 = take(M * D * f);
    L.act = take(M * 2 * f);
    L.lp = take(M * f);
    L.adv = take(M * f);
    L.ret = take(M * f);
    L.val = take(M * f);
    L.ident = take(M * (int64_t)sizeof(int64_t));
    L.parts = take((int64_t)evac::kTfgMaxBlocks * evac::tfg_parts(M) * evac::kTfgPart * f);
    L.total = o;
    return L;
}

// What evac_transformer_minibatch_grad checks and sets up: rpo_prepare's, then the encoder's sizes before its pointers, and the
// fields of TfgArgs that do not depend on the minibatch.  `a` is left as rpo_prepare leaves it: reading the CALLER'S batch.
inline int transformer_prepare(const evac_mlp_policy_t* policy, const evac_transformer_t* encoder, const evac_rpo_loss_config_t* cfg,
                               int64_t batch_size, const float* b_obs, const float* b_actions, const float* b_logprobs,
                               const float* b_advantages, const float* b_returns, const float* b_values, int64_t n_minibatch,
                               const int64_t* mb_inds, const float* rpo_noise, uint64_t seed, const evac_mlp_policy_grads_t* grads_out,
                               const evac_transformer_grads_t* encoder_grads_out, float* stats_out, void* workspace, evac::RpoArgs& a,
                               evac::TfgArgs& s) {
    if (const int rc = rpo_prepare(policy, cfg, batch_size, b_obs, b_actions, b_logprobs, b_advantages, b_returns, b_values, n_minibatch,
                                   mb_inds, rpo_noise, seed, grads_out, stats_out, workspace, a);
        rc != EVAC_OK)
        return rc;
    if (!encoder || !encoder_grads_out) return EVAC_ERR_INVALID_ARGUMENT;
    const evac_transformer_t& T = *encoder;
    std::string why;
    if (const int rc = transformer_check_sizes(T, why); rc != EVAC_OK) return rc;
    const int D = a.D, dm = T.elem_dim;
    if (dm < 1 || dm > kTransformerMaxModelDim || D % dm != 0 || D / dm < 3) return EVAC_ERR_INVALID_ARGUMENT;   // (N + 2 tokens, N >= 1)
    if (D / dm > kTransformerMaxTokens) return EVAC_ERR_UNSUPPORTED;                                             // (one wave holds them)
    if (const int rc = transformer_check_blocks(T, why); rc != EVAC_OK) return rc;
    for (int b = 0; b < T.num_blocks; ++b)
        if (!transformer_block_all_set(encoder_grads_out->blocks[b])) return EVAC_ERR_INVALID_ARGUMENT;
    s = evac::TfgArgs{};
    for (int b = 0; b < T.num_blocks; ++b) {
        const float* const* w = &T.blocks[b].wq;                   // (16 pointers in order: asserted above)
        float* const* g = &encoder_grads_out->blocks[b].wq;
        for (int i = 0; i < evac::kTfgTensors; ++i) {
            s.blk[b].w[i] = w[i];
            s.blk[b].g[i] = g[i];
        }
    }
    s.w1a = policy->actor_w1; s.w1c = policy->critic_w1;
    s.obs = b_obs; s.actions = b_actions; s.logprobs = b_logprobs; s.adv = b_advantages; s.ret = b_returns; s.val = b_values;
    s.B = batch_size;
    s.D = D; s.dm = dm; s.S = D / dm; s.nb = T.num_blocks; s.resid = T.use_resid != 0;
    return EVAC_OK;
}
// One minibatch step: fills the fields of `s` that depend on the step (rpo_shape has shaped `step`) and returns the arguments of
// k_rpo_*: the actor-critic reads the encoded batch, M rows in minibatch order, every one of them in the minibatch.
inline evac::RpoArgs transformer_step(evac::RpoArgs step, evac::TfgArgs& s) {
    const int D = step.D;
    const int64_t M = step.M;
    const TfgLayout L = tfg_layout(D, M);
    char* ws = step.ws;
    s.inds = step.inds;
    s.Y = (float*)(ws + L.Y); s.dX = (float*)(ws + L.dX); s.X1 = (float*)(ws + L.X1);
    s.act_g = (float*)(ws + L.act); s.lp_g = (float*)(ws + L.lp); s.adv_g = (float*)(ws + L.adv); s.ret_g = (float*)(ws + L.ret);
    s.val_g = (float*)(ws + L.val);
    s.ident = (int64_t*)(ws + L.ident);
    s.g1 = (const float*)(ws + evac::kWsFixedBytes);                          // (ws_g1 of the inner workspace)
    s.parts = (float*)(ws + L.parts);
    s.tickets = (unsigned*)(ws + L.header);
    s.slots = (float*)(ws + L.header + 64);
    s.stats = step.stats;
    s.M = (int)M;
    const int p0 = evac::tfg_parts(M);
    s.chunk = (int)((M + p0 - 1) / p0);
    s.P = (int)((M + s.chunk - 1) / s.chunk);                                 // (P <= p0: the workspace's bound)
    step.obs = s.Y; step.actions = s.act_g; step.logprobs = s.lp_g; step.adv = s.adv_g; step.ret = s.ret_g; step.val = s.val_g;
    step.inds = s.ident;
    step.B = M;
    return step;
}

// The launches of one minibatch's gradient, all 13 + 16 num_blocks tensors.
inline void transformer_launch(const evac::RpoArgs& a, const evac::TfgArgs& s, hipStream_t S) {
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

}  // namespace

extern "C" {

int64_t evac_transformer_workspace_bytes(int32_t obs_dim, int64_t n_minibatch) {
    if (evac_rpo_workspace_bytes(obs_dim, n_minibatch) < 0) return EVAC_ERR_INVALID_ARGUMENT;
    return tfg_layout(obs_dim, n_minibatch).total;
}

int evac_transformer_minibatch_grad(const evac_mlp_policy_t* policy, const evac_transformer_t* encoder, const evac_rpo_loss_config_t* cfg,
                                    int64_t batch_size, const float* b_obs, const float* b_actions, const float* b_logprobs,
                                    const float* b_advantages, const float* b_returns, const float* b_values, int64_t n_minibatch,
                                    const int64_t* mb_inds, const float* rpo_noise, uint64_t seed, uint64_t draw_counter,
                                    const evac_mlp_policy_grads_t* grads_out, const evac_transformer_grads_t* encoder_grads_out,
                                    float* stats_out, void* workspace, void* stream) {
    evac::RpoArgs a;
    evac::TfgArgs s;
    if (const int rc = transformer_prepare(policy, encoder, cfg, batch_size, b_obs, b_actions, b_logprobs, b_advantages, b_returns,
                                           b_values, n_minibatch, mb_inds, rpo_noise, seed, grads_out, encoder_grads_out, stats_out,
                                           workspace, a, s);
        rc != EVAC_OK)
        return rc;
    rpo_shape(a, n_minibatch, draw_counter);
    const evac::RpoArgs inner = transformer_step(a, s);
    const int dev = device_of(workspace);
    DeviceGuard g(dev);
    if (rpo_raise_lds<evac::k_rpo_grad<>>(a.D, dev) != EVAC_OK) return EVAC_ERR_HIP;
    transformer_launch(inner, s, (hipStream_t)stream);
    return hipGetLastError() == hipSuccess ? EVAC_OK : EVAC_ERR_HIP;
}

}  // extern "C"
