// Host side of the deep-sets leader's training entries, the part its two translation units share (evac_deepsets_train_api.hip:
// the gradient; evac_deepsets_update_api.hip: the gradient with the optimiser, and the whole update): the workspace's layout, what
// the entries check of their arguments, the kernels' argument structs and the launches of one minibatch's gradient.
#pragma once

#include "evac_deepsets_train.h"
#include "evac_train_host.h"

static_assert(evac::kSetTrainHidden == kSetEncoderHidden && evac::kSetTrainMaxElemDim == kSetEncoderMaxElemDim,
              "deepsets_check: the widths the gradient's kernels take, which are the rollout's (evac_deepsets_api.hip asserts its own)");

namespace {

constexpr int64_t kSetAlign = 256;
inline int64_t set_round_up(int64_t n) { return (n + kSetAlign - 1) / kSetAlign * kSetAlign; }

// The workspace: evac_rpo_minibatch_grad's own (for a batch of M rows of D floats) | tickets and slots | Y | dY | s | t | the
// gathered actions, log-probabilities, advantages, returns, values | the index vector | the partials | the dW_r segments;
// every part on a 256-byte boundary.
struct SetLayout {
    int64_t header, Y, dY, sv, tv, act, lp, adv, ret, val, ident, parts, rparts, total;
};
inline SetLayout set_layout(int32_t D, int64_t M) {
    SetLayout L;
    int64_t o = set_round_up(evac_rpo_workspace_bytes(D, M));
    const auto take = [&o](int64_t bytes) {
        const int64_t at = o;
        o += set_round_up(bytes);
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

// What evac_deepsets_minibatch_grad checks and sets up: rpo_prepare's, the encoder's, and the fields of SetArgs that do not
// depend on the minibatch.  `a` is left as rpo_prepare leaves it: reading the CALLER'S batch.
inline int deepsets_prepare(const evac_mlp_policy_t* policy, const evac_deepsets_t* encoder, const evac_rpo_loss_config_t* cfg,
                            int64_t batch_size, const float* b_obs, const float* b_actions, const float* b_logprobs,
                            const float* b_advantages, const float* b_returns, const float* b_values, int64_t n_minibatch,
                            const int64_t* mb_inds, const float* rpo_noise, uint64_t seed, const evac_mlp_policy_grads_t* grads_out,
                            const evac_deepsets_grads_t* encoder_grads_out, float* stats_out, void* workspace, evac::RpoArgs& a,
                            evac::SetArgs& s) {
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
    s = evac::SetArgs{};
    s.phi_w1 = E.phi_w1; s.phi_b1 = E.phi_b1; s.phi_w2 = E.phi_w2; s.phi_b2 = E.phi_b2; s.rho_w = E.rho_w; s.rho_b = E.rho_b;
    s.g_phi_w1 = G.phi_w1; s.g_phi_b1 = G.phi_b1; s.g_phi_w2 = G.phi_w2; s.g_phi_b2 = G.phi_b2; s.g_rho_w = G.rho_w; s.g_rho_b = G.rho_b;
    s.w1a = policy->actor_w1; s.w1c = policy->critic_w1;
    s.obs = b_obs; s.actions = b_actions; s.logprobs = b_logprobs; s.adv = b_advantages; s.ret = b_returns; s.val = b_values;
    s.B = batch_size;
    s.D = D; s.ed = ed; s.S = D / ed;
    return EVAC_OK;
}
// One minibatch step: `step` is rpo_prepare's arguments shaped for the step (rpo_shape: M samples at step.inds of the caller's
// batch, statistics to step.stats).  Fills the fields of `s` that depend on the step and returns the arguments of k_rpo_*: the
// actor-critic reads the encoded batch, M rows in minibatch order, every one of them in the minibatch.
inline evac::RpoArgs deepsets_step(evac::RpoArgs step, evac::SetArgs& s) {
    const int D = step.D;
    const int64_t M = step.M;
    const SetLayout L = set_layout(D, M);
    char* ws = step.ws;
    s.inds = step.inds;
    s.Y = (float*)(ws + L.Y); s.dY = (float*)(ws + L.dY); s.sv = (float*)(ws + L.sv); s.tv = (float*)(ws + L.tv);
    s.act_g = (float*)(ws + L.act); s.lp_g = (float*)(ws + L.lp); s.adv_g = (float*)(ws + L.adv); s.ret_g = (float*)(ws + L.ret);
    s.val_g = (float*)(ws + L.val);
    s.ident = (int64_t*)(ws + L.ident);
    s.g1 = (const float*)(ws + evac::kWsFixedBytes);                          // (ws_g1 of the inner workspace)
    s.parts = (float*)(ws + L.parts); s.rparts = (float*)(ws + L.rparts);
    s.tickets = (unsigned*)(ws + L.header);
    s.slots = (float*)(ws + L.header + 64);
    s.stats = step.stats;
    s.M = (int)M;
    const int p0 = evac::set_parts(M);
    s.chunk = (int)((M + p0 - 1) / p0);
    s.chunk = (s.chunk + evac::kSetTile - 1) / evac::kSetTile * evac::kSetTile;   // whole tiles: every workgroup but the last
    s.P = (int)((M + s.chunk - 1) / s.chunk);                                     // (P <= p0: the workspace's bound)
    s.Sr = evac::set_segments(M);
    s.seglen = (int)((M + s.Sr - 1) / s.Sr);
    step.obs = s.Y; step.actions = s.act_g; step.logprobs = s.lp_g; step.adv = s.adv_g; step.ret = s.ret_g; step.val = s.val_g;
    step.inds = s.ident;
    step.B = M;
    return step;
}

// The launches of one minibatch's gradient, all 19 tensors: the encoder forwards, rpo_launch on the encoded observations, the
// encoder backwards, its finish.  `gate` as rpo_launch's.
template <class... Gate>
inline void deepsets_launch(const evac::RpoArgs& a, const evac::SetArgs& s, hipStream_t S, Gate... gate) {
    const int64_t M = s.M;
    const int64_t enc_wgs = (M + evac::kSetWaves - 1) / evac::kSetWaves;
    hipLaunchKernelGGL(evac::k_set_encode<Gate...>, dim3((unsigned)(enc_wgs > evac::kSetEncodeMaxWgs ? evac::kSetEncodeMaxWgs : enc_wgs)),
                       dim3(evac::kSetBlock), 0, S, s, gate...);
    rpo_launch(a, S, gate...);
    hipLaunchKernelGGL(evac::k_set_backward<Gate...>, dim3((unsigned)s.P), dim3(evac::kSetBlock), 0, S, s, gate...);
    const int rtiles = (s.D + evac::kSetRTile - 1) / evac::kSetRTile;
    hipLaunchKernelGGL(evac::k_set_finish<Gate...>, dim3((unsigned)(rtiles * s.Sr + 1)), dim3(evac::kSetBlock), 0, S, s, gate...);
}

}  // namespace
