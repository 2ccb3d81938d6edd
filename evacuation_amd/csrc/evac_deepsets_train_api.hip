// Host side of the deep-sets leader's gradient (include/evac.h: evac_deepsets_workspace_bytes, evac_deepsets_minibatch_grad;
// kernels in evac_deepsets_train.h and, launched as they are, evac_train.h's k_rpo_*<>): argument checking, the workspace's
// layout and six launches.  No handle: errors come back through the return code alone and every refusal comes before the first
// HIP call.  No device allocation, no synchronisation: the call only enqueues work on the caller's stream.
#include <hip/hip_runtime.h>

#include <cstddef>
#include <cstdint>

#include "evac_deepsets_train.h"
#include "evac_train_host.h"

static_assert(evac::kSetTrainHidden == kSetEncoderHidden && evac::kSetTrainMaxElemDim == kSetEncoderMaxElemDim,
              "deepsets_check: the widths the gradient's kernels take, which are the rollout's (evac_deepsets_api.hip asserts its own)");

namespace {

constexpr int64_t kAlign = 256;
inline int64_t round_up(int64_t n) { return (n + kAlign - 1) / kAlign * kAlign; }

// The workspace: evac_rpo_minibatch_grad's own (for a batch of M rows of D floats) | tickets and slots | Y | dY | s | t | the
// gathered actions, log-probabilities, advantages, returns, values | the index vector | the partials | the dW_r segments;
// every part on a 256-byte boundary.
struct SetLayout {
    int64_t header, Y, dY, sv, tv, act, lp, adv, ret, val, ident, parts, rparts, total;
};
inline SetLayout set_layout(int32_t D, int64_t M) {
    SetLayout L;
    int64_t o = round_up(evac_rpo_workspace_bytes(D, M));
    const auto take = [&o](int64_t bytes) {
        const int64_t at = o;
        o += round_up(bytes);
        return at;
    };
    const int64_t f = (int64_t)sizeof(float);
    L.header = take(evac::kSetHeaderBytes);
    L.Y = take(M * D * f);
    L.dY = take(M * D * f);
    L.sv = take(M * evac::kSetTrainHidden * f);
    L.tv = take(M * evac::kSetTrainHidden * f);
    L.act = take(M * 2 * f);
    L.lp = take(M * f);
    L.adv = take(M * f);
    L.ret = take(M * f);
    L.val = take(M * f);
    L.ident = take(M * (int64_t)sizeof(int64_t));
    L.parts = take((int64_t)evac::set_parts(M) * evac::kSetPart * f);
    const int64_t tiles = (D + evac::kSetRTile - 1) / evac::kSetRTile;
    L.rparts = take(tiles * evac::set_segments(M) * evac::kSetRRows * evac::kSetRTile * f);
    L.total = o;
    return L;
}

}  // namespace

extern "C" {

int64_t evac_deepsets_workspace_bytes(int32_t obs_dim, int64_t n_minibatch) {
    if (evac_rpo_workspace_bytes(obs_dim, n_minibatch) < 0) return EVAC_ERR_INVALID_ARGUMENT;
    return set_layout(obs_dim, n_minibatch).total;
}

int evac_deepsets_minibatch_grad(const evac_mlp_policy_t* policy, const evac_deepsets_t* encoder, const evac_rpo_loss_config_t* cfg,
                                 int64_t batch_size, const float* b_obs, const float* b_actions, const float* b_logprobs,
                                 const float* b_advantages, const float* b_returns, const float* b_values, int64_t n_minibatch,
                                 const int64_t* mb_inds, const float* rpo_noise, uint64_t seed, uint64_t draw_counter,
                                 const evac_mlp_policy_grads_t* grads_out, const evac_deepsets_grads_t* encoder_grads_out,
                                 float* stats_out, void* workspace, void* stream) {
    evac::RpoArgs a;
    if (const int rc = rpo_prepare(policy, cfg, batch_size, b_obs, b_actions, b_logprobs, b_advantages, b_returns, b_values, n_minibatch,
                                   mb_inds, rpo_noise, seed, grads_out, stats_out, workspace, a);
        rc != EVAC_OK)
        return rc;
    if (!encoder || !encoder_grads_out) return EVAC_ERR_INVALID_ARGUMENT;
    const evac_deepsets_t& E = *encoder;
    const evac_deepsets_grads_t& G = *encoder_grads_out;
    if (!G.phi_w1 || !G.phi_b1 || !G.phi_w2 || !G.phi_b2 || !G.rho_w || !G.rho_b) return EVAC_ERR_INVALID_ARGUMENT;
    const int D = a.D, ed = E.set_elem_dim;
    const bool rows_fit = ed > 0 && D % ed == 0 && D / ed >= 3;             // (N + 2 rows, N >= 1)
    if (!deepsets_check(E, D, 0, rows_fit).empty()) return EVAC_ERR_INVALID_ARGUMENT;

    const int64_t M = n_minibatch;
    const SetLayout L = set_layout(D, M);
    char* ws = (char*)workspace;
    evac::SetArgs s{};
    s.phi_w1 = E.phi_w1; s.phi_b1 = E.phi_b1; s.phi_w2 = E.phi_w2; s.phi_b2 = E.phi_b2; s.rho_w = E.rho_w; s.rho_b = E.rho_b;
    s.g_phi_w1 = G.phi_w1; s.g_phi_b1 = G.phi_b1; s.g_phi_w2 = G.phi_w2; s.g_phi_b2 = G.phi_b2; s.g_rho_w = G.rho_w; s.g_rho_b = G.rho_b;
    s.w1a = policy->actor_w1; s.w1c = policy->critic_w1;
    s.obs = b_obs; s.actions = b_actions; s.logprobs = b_logprobs; s.adv = b_advantages; s.ret = b_returns; s.val = b_values;
    s.inds = mb_inds;
    s.B = batch_size;
    s.Y = (float*)(ws + L.Y); s.dY = (float*)(ws + L.dY); s.sv = (float*)(ws + L.sv); s.tv = (float*)(ws + L.tv);
    s.act_g = (float*)(ws + L.act); s.lp_g = (float*)(ws + L.lp); s.adv_g = (float*)(ws + L.adv); s.ret_g = (float*)(ws + L.ret);
    s.val_g = (float*)(ws + L.val);
    s.ident = (int64_t*)(ws + L.ident);
    s.g1 = (const float*)(ws + evac::kWsFixedBytes);                          // (ws_g1 of the inner workspace)
    s.parts = (float*)(ws + L.parts); s.rparts = (float*)(ws + L.rparts);
    s.tickets = (unsigned*)(ws + L.header);
    s.slots = (float*)(ws + L.header + 64);
    s.stats = stats_out;
    s.D = D; s.M = (int)M; s.ed = ed; s.S = D / ed;
    const int p0 = evac::set_parts(M);
    s.chunk = (int)((M + p0 - 1) / p0);
    s.chunk = (s.chunk + evac::kSetTile - 1) / evac::kSetTile * evac::kSetTile;   // whole tiles: every workgroup but the last
    s.P = (int)((M + s.chunk - 1) / s.chunk);                                     // (P <= p0: the workspace's bound)
    s.Sr = evac::set_segments(M);
    s.seglen = (int)((M + s.Sr - 1) / s.Sr);

    // the actor-critic reads the encoded batch: M rows in minibatch order, every one of them in the minibatch
    a.obs = s.Y; a.actions = s.act_g; a.logprobs = s.lp_g; a.adv = s.adv_g; a.ret = s.ret_g; a.val = s.val_g;
    a.inds = s.ident;
    a.B = M;
    rpo_shape(a, M, draw_counter);

    const int dev = device_of(workspace);
    DeviceGuard g(dev);
    if (rpo_raise_lds<evac::k_rpo_grad<>>(D, dev) != EVAC_OK) return EVAC_ERR_HIP;
    hipStream_t S = (hipStream_t)stream;
    const int64_t enc_wgs = (M + evac::kSetWaves - 1) / evac::kSetWaves;
    hipLaunchKernelGGL(evac::k_set_encode, dim3((unsigned)(enc_wgs > evac::kSetEncodeMaxWgs ? evac::kSetEncodeMaxWgs : enc_wgs)),
                       dim3(evac::kSetBlock), 0, S, s);
    rpo_launch(a, S);
    hipLaunchKernelGGL(evac::k_set_backward, dim3((unsigned)s.P), dim3(evac::kSetBlock), 0, S, s);
    const int rtiles = (D + evac::kSetRTile - 1) / evac::kSetRTile;
    hipLaunchKernelGGL(evac::k_set_finish, dim3((unsigned)(rtiles * s.Sr + 1)), dim3(evac::kSetBlock), 0, S, s);
    return hipGetLastError() == hipSuccess ? EVAC_OK : EVAC_ERR_HIP;
}

}  // extern "C"
