// Host side of the gradient behind an encoder, the part the deep-sets and the transformer leader's entries share
// (evac_deepsets_train_api.hip, evac_deepsets_update_api.hip, evac_transformer_train_api.hip, evac_transformer_update_api.hip):
// the workspace's cursor and its gathered columns, the halves of "prepare" and "step" that are the same in front of either
// encoder, the sizer's body and the whole body of a gradient entry.  What differs sits in a trait per encoder (SetGrad in evac_deepsets_train_host.h, TfGrad in
// evac_transformer_train_host.h):
//
//   Encoder, Grads, Args      the C structs and the kernels' argument struct (evac::SetArgs / evac::TfgArgs, whose equally named
//                             fields the templates here reach by name: the two share no base, which would move kernel arguments)
//   Layout, layout(D, M)      the workspace's parts; `header`, `Y`, `cols`, `parts` and `total` are read here
//   check(E, G, D, s)         the encoder's own refusals in its own order, then `s` = Args{} with the encoder's own fields
//   shape(s, L, ws, M)        the encoder's own parts of the workspace and its own step fields (chunk, P, ..)
//   launch(a, s, S, gate...)  the launches of one minibatch's gradient
#pragma once

#include "evac_train_host.h"

namespace {

// The workspace behind evac_rpo_minibatch_grad's own: every part on a 256-byte boundary.
constexpr int64_t kWsAlign = 256;
inline int64_t ws_round_up(int64_t n) { return (n + kWsAlign - 1) / kWsAlign * kWsAlign; }
struct WsCursor {
    int64_t o;
    int64_t take(int64_t bytes) {
        const int64_t at = o;
        o += ws_round_up(bytes);
        return at;
    }
};
// ... which starts where the inner workspace (for a batch of M rows of D floats) ends
inline WsCursor encoder_ws_cursor(int32_t D, int64_t M) { return WsCursor{ws_round_up(evac_rpo_workspace_bytes(D, M))}; }

// The gathered actions, log-probabilities, advantages, returns, values | the index vector
struct GatheredLayout {
    int64_t act, lp, adv, ret, val, ident;
};
inline GatheredLayout take_gathered(WsCursor& c, int64_t M) {
    const int64_t f = (int64_t)sizeof(float);
    GatheredLayout L;
    L.act = c.take(M * 2 * f);
    L.lp = c.take(M * f);
    L.adv = c.take(M * f);
    L.ret = c.take(M * f);
    L.val = c.take(M * f);
    L.ident = c.take(M * (int64_t)sizeof(int64_t));
    return L;
}

template <class Enc>
inline int64_t encoder_workspace_bytes(int32_t obs_dim, int64_t n_minibatch) {
    if (evac_rpo_workspace_bytes(obs_dim, n_minibatch) < 0) return EVAC_ERR_INVALID_ARGUMENT;
    return Enc::layout(obs_dim, n_minibatch).total;
}

// The fields of SetArgs / TfgArgs that name the CALLER'S batch and the first layers that read the encoded one.
template <class Args>
inline void encoder_grad_fill_batch(Args& s, const evac_mlp_policy_t* policy, const float* b_obs, const float* b_actions,
                                    const float* b_logprobs, const float* b_advantages, const float* b_returns, const float* b_values,
                                    int64_t batch_size) {
    s.w1a = policy->actor_w1; s.w1c = policy->critic_w1;
    s.obs = b_obs; s.actions = b_actions; s.logprobs = b_logprobs; s.adv = b_advantages; s.ret = b_returns; s.val = b_values;
    s.B = batch_size;
}
// The fields of `s` that every encoder's step points into the workspace; returns the arguments of k_rpo_*: the actor-critic reads
// the encoded batch, M rows in minibatch order, every one of them in the minibatch.
template <class Args, class Layout>
inline evac::RpoArgs encoder_grad_point_step(evac::RpoArgs step, Args& s, const Layout& L) {
    char* ws = step.ws;
    s.inds = step.inds;
    s.Y = (float*)(ws + L.Y);
    s.act_g = (float*)(ws + L.cols.act); s.lp_g = (float*)(ws + L.cols.lp); s.adv_g = (float*)(ws + L.cols.adv);
    s.ret_g = (float*)(ws + L.cols.ret); s.val_g = (float*)(ws + L.cols.val);
    s.ident = (int64_t*)(ws + L.cols.ident);
    s.g1 = (const float*)(ws + evac::kWsFixedBytes);                          // (ws_g1 of the inner workspace)
    s.parts = (float*)(ws + L.parts);
    s.tickets = (unsigned*)(ws + L.header);
    s.slots = (float*)(ws + L.header + 64);
    s.stats = step.stats;
    s.M = step.M;
    step.obs = s.Y; step.actions = s.act_g; step.logprobs = s.lp_g; step.adv = s.adv_g; step.ret = s.ret_g; step.val = s.val_g;
    step.inds = s.ident;
    step.B = step.M;
    return step;
}

// What an encoder's gradient entry checks and sets up: rpo_prepare's, then the encoder's (Enc::check), and the fields of `s` that
// do not depend on the minibatch.  `a` is left as rpo_prepare leaves it: reading the CALLER'S batch.
template <class Enc>
inline int encoder_grad_prepare(const evac_mlp_policy_t* policy, const typename Enc::Encoder* encoder, const evac_rpo_loss_config_t* cfg,
                                int64_t batch_size, const float* b_obs, const float* b_actions, const float* b_logprobs,
                                const float* b_advantages, const float* b_returns, const float* b_values, int64_t n_minibatch,
                                const int64_t* mb_inds, const float* rpo_noise, uint64_t seed, const evac_mlp_policy_grads_t* grads_out,
                                const typename Enc::Grads* encoder_grads_out, float* stats_out, void* workspace, evac::RpoArgs& a,
                                typename Enc::Args& s) {
    if (const int rc = rpo_prepare(policy, cfg, batch_size, b_obs, b_actions, b_logprobs, b_advantages, b_returns, b_values, n_minibatch,
                                   mb_inds, rpo_noise, seed, grads_out, stats_out, workspace, a);
        rc != EVAC_OK)
        return rc;
    if (!encoder || !encoder_grads_out) return EVAC_ERR_INVALID_ARGUMENT;
    if (const int rc = Enc::check(*encoder, *encoder_grads_out, a.D, s); rc != EVAC_OK) return rc;
    encoder_grad_fill_batch(s, policy, b_obs, b_actions, b_logprobs, b_advantages, b_returns, b_values, batch_size);
    return EVAC_OK;
}
// One minibatch step: `step` is rpo_prepare's arguments shaped for the step (rpo_shape: M samples at step.inds of the caller's
// batch, statistics to step.stats).  Fills the fields of `s` that depend on the step and returns the arguments of k_rpo_*.
template <class Enc>
inline evac::RpoArgs encoder_grad_step(const evac::RpoArgs& step, typename Enc::Args& s) {
    const typename Enc::Layout L = Enc::layout(step.D, step.M);
    Enc::shape(s, L, step.ws, step.M);
    return encoder_grad_point_step(step, s, L);
}

// The scalars of `o` (adam_prepare's, then set for a step by rpo_update_steps) into an encoder's optimiser arguments
// (evac::SetAdamArgs, evac::TfAdamArgs: the fields AdamArgs names, under the same names).
template <class EncAdamArgs>
inline void encoder_adam_scalars(const evac::AdamArgs& o, EncAdamArgs& q) {
    q.hdr = o.hdr; q.sumsq = o.sumsq; q.stats = o.stats;
    q.lr = o.lr; q.beta1 = o.beta1; q.beta2 = o.beta2; q.target_kl = o.target_kl;
    q.max_norm = o.max_norm; q.w = o.w; q.b2 = o.b2; q.u = o.u; q.eps = o.eps;
    q.gated = o.gated; q.epoch_last = o.epoch_last; q.use_target_kl = o.use_target_kl;
}

// What follows the gradient in the same call: nothing (the step's entry: the optimiser's checks, and its launch).
struct NothingMore {
    int operator()() const { return EVAC_OK; }
    void operator()(hipStream_t) const {}
};
// The whole body of evac_deepsets_minibatch_grad / evac_transformer_minibatch_grad.  `check()` adds refusals behind the
// gradient's own and before the first HIP call; `then(stream)` enqueues behind the gradient's launches.
template <class Enc, class Check = NothingMore, class Then = NothingMore>
inline int encoder_minibatch_grad(const evac_mlp_policy_t* policy, const typename Enc::Encoder* encoder, const evac_rpo_loss_config_t* cfg,
                                  int64_t batch_size, const float* b_obs, const float* b_actions, const float* b_logprobs,
                                  const float* b_advantages, const float* b_returns, const float* b_values, int64_t n_minibatch,
                                  const int64_t* mb_inds, const float* rpo_noise, uint64_t seed, uint64_t draw_counter,
                                  const evac_mlp_policy_grads_t* grads_out, const typename Enc::Grads* encoder_grads_out,
                                  float* stats_out, void* workspace, void* stream, Check check = Check{}, Then then = Then{}) {
    evac::RpoArgs a;
    typename Enc::Args s;
    if (const int rc = encoder_grad_prepare<Enc>(policy, encoder, cfg, batch_size, b_obs, b_actions, b_logprobs, b_advantages, b_returns,
                                                 b_values, n_minibatch, mb_inds, rpo_noise, seed, grads_out, encoder_grads_out,
                                                 stats_out, workspace, a, s);
        rc != EVAC_OK)
        return rc;
    if (const int rc = check(); rc != EVAC_OK) return rc;
    rpo_shape(a, n_minibatch, draw_counter);
    const evac::RpoArgs inner = encoder_grad_step<Enc>(a, s);
    const int dev = device_of(workspace);
    DeviceGuard g(dev);
    if (rpo_raise_lds<evac::k_rpo_grad<>>(a.D, dev) != EVAC_OK) return EVAC_ERR_HIP;
    Enc::launch(inner, s, (hipStream_t)stream);
    then((hipStream_t)stream);
    return hipGetLastError() == hipSuccess ? EVAC_OK : EVAC_ERR_HIP;
}

}  // namespace
