// Host side of training behind an encoder, the part the deep-sets and the transformer leader's entries share
// (evac_{deepsets,transformer}_train_api.hip: the gradient; evac_{deepsets,transformer}_update_api.hip: the optimiser step, the
// gradient with the optimiser and the whole update; through evac_encoder_population_host.h the two population updates): the
// workspace's cursor and its gathered columns, the halves of "prepare" and "step" that are the same in front of either encoder,
// the sizer's body, the launches of one minibatch's gradient, and the whole bodies of a gradient entry, an optimiser step, a
// minibatch step and an update.  What differs sits in two traits per encoder.
//
// The gradient's (SetGrad in evac_deepsets_train_host.h, TfGrad in evac_transformer_train_host.h):
//   Encoder, Grads, Args      the C structs and the kernels' argument struct (evac::SetArgs / evac::TfgArgs, whose equally named
//                             fields the templates here reach by name: the two share no base, which would move kernel arguments)
//   Layout, layout(D, M)      the workspace's parts; `header`, `Y`, `cols`, `parts` and `total` are read here
//   check(E, G, D, s)         the encoder's own refusals in its own order, then `s` = Args{} with the encoder's own fields
//   shape(s, L, ws, M)        the encoder's own parts of the workspace and its own step fields (chunk, P, ..)
//   encode(s, y, S, tail...)  the encoder's launches in front of the actor-critic's, a grid of y rows (one per learner) ...
//   backward(s, y, S, tail...)   ... and behind them.  `tail` is what the kernels take behind `s`: nothing, the stop gate, or the
//                             gate and the learners' strides; it names the kernels' instantiation.
//   LearnerStrides            those strides (evac::SetLearnerStrides / evac::TfgLearnerStrides)
//
// The optimiser's (SetAdam in evac_deepsets_adam_host.h, TfAdam in evac_transformer_adam_host.h):
//   State, Grads, Args        the C structs and the kernel's argument struct (evac::SetAdamArgs / evac::TfAdamArgs)
//   Dims, dims(E)             the encoder's sizes that size its tensors, from the C struct of the encoder
//   check(D, dims)            the encoder's own size refusals in its own order
//   fresh(dims)               Args{}, with the tensor count where the kernel reads it
//   count(dims), tensor(G, i), size(i, D, dims)   the encoder's tensors behind the actor-critic's 13: how many, the i-th pointer
//                             of a Grads, its elements
//   launch(kernel, q, learners, S, rest...)   one launch of the unit's own kernel (k_adam_* / k_adam_*_population, each defined in
//                             one unit alone) over a grid of `learners` rows
//   Strides, EncoderStrides, strides(E, D, n_learners, p, g, m, sq, aq)   a population's: the population kernel's strides, the C
//                             struct of an encoder's, and the check of the three of them (parameters, gradients, moments) with
//                             their copy into the gradient's LearnerStrides `sq` and into `aq` behind the 13
#pragma once

#include <cstddef>

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

// The launches of one minibatch's gradient: the encoder forwards, rpo_launch on the encoded observations, the encoder backwards.
// `gate` as rpo_launch's.
template <class Enc, class... Gate>
inline void encoder_grad_launch(const evac::RpoArgs& a, const typename Enc::Args& s, hipStream_t S, Gate... gate) {
    Enc::encode(s, 1u, S, gate...);
    rpo_launch(a, S, gate...);
    Enc::backward(s, 1u, S, gate...);
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
    encoder_grad_launch<Enc>(inner, s, (hipStream_t)stream);
    then((hipStream_t)stream);
    return hipGetLastError() == hipSuccess ? EVAC_OK : EVAC_ERR_HIP;
}

// What an encoder's optimiser step checks and sets up: adam_prepare for the 13 tensors (into `o`), then the encoder's -- its
// sizes (Opt::check) before its pointers, parameters, gradients and both moments alike -- and every tensor's elements and
// workgroups.
template <class Opt>
inline int encoder_adam_prepare(const evac_mlp_policy_grads_t* params, const typename Opt::Grads* enc_params,
                                const evac_mlp_policy_grads_t* grads, const typename Opt::Grads* enc_grads,
                                const typename Opt::State* state, const evac_adam_config_t* cfg, int32_t obs_dim,
                                const typename Opt::Dims& dims, evac::AdamArgs& o, typename Opt::Args& q) {
    if (!state || !enc_params || !enc_grads) return EVAC_ERR_INVALID_ARGUMENT;
    const evac_adam_state_t linear{state->header, state->exp_avg, state->exp_avg_sq};
    if (const int rc = adam_prepare(params, grads, &linear, cfg, obs_dim, o); rc != EVAC_OK) return rc;
    if (const int rc = Opt::check(obs_dim, dims); rc != EVAC_OK) return rc;
    q = Opt::fresh(dims);
    const int ne = Opt::count(dims);
    const typename Opt::Grads* sets[4] = {enc_params, enc_grads, &state->enc_exp_avg, &state->enc_exp_avg_sq};
    float* const* lin[4] = {o.p, o.g, o.m, o.v};
    float** dst[4] = {q.p, q.g, q.m, q.v};
    for (int k = 0; k < 4; ++k) {
        for (int i = 0; i < evac::kAdamTensors; ++i) dst[k][i] = lin[k][i];
        for (int i = 0; i < ne; ++i) {
            if (!Opt::tensor(*sets[k], i)) return EVAC_ERR_INVALID_ARGUMENT;
            dst[k][evac::kAdamTensors + i] = Opt::tensor(*sets[k], i);
        }
    }
    int wgs = 0;
    for (int i = 0; i < evac::kAdamTensors + ne; ++i) {
        q.n[i] = i < evac::kAdamTensors ? o.end[i] - (i ? o.end[i - 1] : 0) : Opt::size(i - evac::kAdamTensors, obs_dim, dims);
        q.wg_end[i] = (wgs += (q.n[i] + evac::kAdamBlock - 1) / evac::kAdamBlock);
    }
    encoder_adam_scalars(o, q);
    return EVAC_OK;
}

// The whole body of evac_deepsets_adam_step / evac_transformer_adam_step; `kernel` is the unit's k_adam_set / k_adam_tf.
template <class Opt, class Kernel>
inline int encoder_adam_step(Kernel kernel, const evac_mlp_policy_grads_t* params, const typename Opt::Grads* enc_params,
                             const evac_mlp_policy_grads_t* grads, const typename Opt::Grads* enc_grads, const typename Opt::State* state,
                             const evac_adam_config_t* cfg, int32_t obs_dim, const typename Opt::Dims& dims, const float* grad_sumsq,
                             void* stream) {
    evac::AdamArgs o;
    typename Opt::Args q;
    if (const int rc = encoder_adam_prepare<Opt>(params, enc_params, grads, enc_grads, state, cfg, obs_dim, dims, o, q); rc != EVAC_OK)
        return rc;
    if (!grad_sumsq) return EVAC_ERR_INVALID_ARGUMENT;
    q.sumsq = grad_sumsq;
    DeviceGuard g(device_of(state->header));
    Opt::launch(kernel, q, 1u, (hipStream_t)stream);
    return hipGetLastError() == hipSuccess ? EVAC_OK : EVAC_ERR_HIP;
}

// The whole body of evac_deepsets_minibatch_step / evac_transformer_minibatch_step: encoder_minibatch_grad with the optimiser's
// checks behind the gradient's and its launch behind the gradient's, reading the sum of squares the gradient left at stats_out[7].
template <class Enc, class Opt, class Kernel>
inline int encoder_minibatch_step(Kernel kernel, const evac_mlp_policy_t* policy, const typename Enc::Encoder* encoder,
                                  const evac_rpo_loss_config_t* cfg, int64_t batch_size, const float* b_obs, const float* b_actions,
                                  const float* b_logprobs, const float* b_advantages, const float* b_returns, const float* b_values,
                                  int64_t n_minibatch, const int64_t* mb_inds, const float* rpo_noise, uint64_t seed, uint64_t draw_counter,
                                  const evac_mlp_policy_grads_t* grads_out, const typename Enc::Grads* encoder_grads_out, float* stats_out,
                                  void* workspace, void* stream, const evac_mlp_policy_grads_t* params,
                                  const typename Enc::Grads* enc_params, const typename Opt::State* state,
                                  const evac_adam_config_t* adam_cfg) {
    evac::AdamArgs o;
    typename Opt::Args q;
    return encoder_minibatch_grad<Enc>(
        policy, encoder, cfg, batch_size, b_obs, b_actions, b_logprobs, b_advantages, b_returns, b_values, n_minibatch, mb_inds, rpo_noise,
        seed, draw_counter, grads_out, encoder_grads_out, stats_out, workspace, stream,
        [&] {                                                                  // (behind the gradient's checks: policy and encoder are set)
            const int rc = encoder_adam_prepare<Opt>(params, enc_params, grads_out, encoder_grads_out, state, adam_cfg, policy->obs_dim,
                                                     Opt::dims(*encoder), o, q);
            if (rc == EVAC_OK) q.sumsq = stats_out + 7;
            return rc;
        },
        [&q, kernel](hipStream_t S) { Opt::launch(kernel, q, 1u, S); });
}

// The whole body of evac_deepsets_update / evac_transformer_update: the gradient's checks, the optimiser's, then every step's
// launches (gated by the optimiser's header) over rpo_update_steps.
template <class Enc, class Opt, class Kernel>
inline int encoder_update(Kernel kernel, const evac_mlp_policy_t* policy, const typename Enc::Encoder* encoder,
                          const evac_mlp_policy_grads_t* params, const typename Enc::Grads* enc_params, const evac_mlp_policy_grads_t* grads,
                          const typename Enc::Grads* enc_grads, const evac_rpo_loss_config_t* loss_cfg, const evac_adam_config_t* adam_cfg,
                          const typename Opt::State* state, int64_t batch_size, const float* b_obs, const float* b_actions,
                          const float* b_logprobs, const float* b_advantages, const float* b_returns, const float* b_values,
                          int64_t n_minibatch, int32_t n_epochs, const int64_t* perms, const float* rpo_noise, uint64_t seed,
                          uint64_t first_draw_counter, int32_t use_target_kl, double target_kl, float* stats_out, void* workspace,
                          void* stream) {
    if (n_epochs < 1) return EVAC_ERR_INVALID_ARGUMENT;
    evac::RpoArgs a;
    typename Enc::Args s;
    if (const int rc = encoder_grad_prepare<Enc>(policy, encoder, loss_cfg, batch_size, b_obs, b_actions, b_logprobs, b_advantages,
                                                 b_returns, b_values, n_minibatch, perms, rpo_noise, seed, grads, enc_grads, stats_out,
                                                 workspace, a, s);
        rc != EVAC_OK)
        return rc;
    evac::AdamArgs o;
    typename Opt::Args q;
    if (const int rc = encoder_adam_prepare<Opt>(params, enc_params, grads, enc_grads, state, adam_cfg, policy->obs_dim,
                                                 Opt::dims(*encoder), o, q);
        rc != EVAC_OK)
        return rc;
    o.gated = 1;
    o.use_target_kl = use_target_kl != 0;
    o.target_kl = target_kl;
    const int dev = device_of(workspace);
    DeviceGuard g(dev);
    if (rpo_raise_lds<evac::k_rpo_grad<const evac::AdamHeader*>>(a.D, dev) != EVAC_OK) return EVAC_ERR_HIP;
    hipStream_t S = (hipStream_t)stream;
    // stop, steps_run, epochs_run (and the ticket, zero anyway)
    if (hipMemsetAsync((char*)state->header + offsetof(evac::AdamHeader, stop), 0, 16, S) != hipSuccess) {
        (void)hipGetLastError();
        return EVAC_ERR_HIP;
    }
    rpo_update_steps(a, o, batch_size, n_minibatch, n_epochs, perms, rpo_noise, stats_out, first_draw_counter,
                     [&s, &q, S, kernel](const evac::RpoArgs& step, const evac::AdamArgs& adam, uint64_t) {
                         const evac::RpoArgs inner = encoder_grad_step<Enc>(step, s);
                         encoder_adam_scalars(adam, q);
                         encoder_grad_launch<Enc>(inner, s, S, (const evac::AdamHeader*)adam.hdr);
                         Opt::launch(kernel, q, 1u, S);
                     });
    return hipGetLastError() == hipSuccess ? EVAC_OK : EVAC_ERR_HIP;
}

}  // namespace
