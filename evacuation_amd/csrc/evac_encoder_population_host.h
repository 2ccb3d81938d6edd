// Host side of the update of a population of leaders with an encoder, the part the deep-sets and the transformer population's
// units share (evac_deepsets_population_api.hip, evac_transformer_population_update_api.hip): the workspace's layout and sizer
// and the whole body of the update, over the encoder's two traits of evac_encoder_train_host.h (Enc: SetGrad / TfGrad; Opt:
// SetAdam / TfAdam).  The update is the lone update's checks (encoder_grad_prepare, encoder_adam_prepare) and
// evac_rpo_update_population's (population_prepare) over one step loop (rpo_update_steps), with the learner as one more grid
// dimension of each launch: Enc's launches around evac_population_host.h's three, then Opt's with the unit's own kernel.  Of a
// population the traits add Enc::LearnerStrides, Opt::Strides, Opt::EncoderStrides (the C struct) and Opt::strides(..), the
// check of the encoder's strides and their copy into the other two.  Every refusal before the first HIP call, no device
// allocation, no synchronisation.
// A SWEEP of such a population (evac_deepsets_sweep_api.hip, evac_transformer_sweep_api.hip) is the same body with the learners'
// values from evac_learner_hyper_t: the loss coefficients by value into evac_sweep_api.hip's gradient and finish
// (evac_sweep_host.h), the optimiser's through a table at the workspace's tail that one launch per call fills
// (evac_encoder_sweep.h), read by the unit's k_adam_*_sweep.
#pragma once

#include "evac_encoder_sweep.h"
#include "evac_encoder_train_host.h"
#include "evac_population_host.h"
#include "evac_sweep_host.h"

static_assert(sizeof(evac::RpoArgs) + sizeof(evac::LearnerStrides) + sizeof(evac::LearnerDraws) + sizeof(void*) <= 4096,
              "the gradient kernels' arguments must fit the kernel-argument segment");
static_assert(sizeof(evac::RpoArgs) + sizeof(evac::LearnerStrides) + sizeof(evac::LearnerDraws) + sizeof(evac::LearnerLoss) +
                      sizeof(void*) <= 4096, "the sweep's gradient kernels' arguments must fit the kernel-argument segment");
static_assert(sizeof(evac::LearnerSteps) + sizeof(void*) <= 4096, "k_learner_steps_table: arguments beyond the kernel-argument segment");
static_assert(kWsAlign % kSliceAlign == 0, "slices of whole 256-byte parts: no two learners share a 128-byte line");

namespace {

// The workspace: S slices of the lone learner's (Enc::layout: every part on a 256-byte boundary, its Y and gathered columns left
// unused), then what the actor-critic's kernels read as one common batch of S x M rows: Y | the gathered actions,
// log-probabilities, advantages, returns, values | the index lists.  A step of m <= M samples packs the learners' rows densely:
// learner s's begin s x m rows into each part.
struct PopulationLayout {
    int64_t slice, Y;
    GatheredLayout cols;
    int64_t total;
};
template <class Enc>
inline PopulationLayout encoder_population_layout(int32_t D, int64_t M, int64_t S) {
    PopulationLayout L;
    L.slice = ws_round_up(Enc::layout(D, M).total);
    WsCursor c{L.slice * S};
    L.Y = c.take(S * M * D * (int64_t)sizeof(float));
    L.cols = take_gathered(c, S * M);
    L.total = c.o;
    return L;
}

// The whole body of evac_deepsets_population_workspace_bytes / evac_transformer_population_workspace_bytes.
template <class Enc>
inline int64_t encoder_population_workspace_bytes(int32_t obs_dim, int64_t n_minibatch, int32_t n_learners) {
    if (n_learners < 1 || n_learners > EVAC_MAX_LEARNERS) return EVAC_ERR_INVALID_ARGUMENT;
    if (encoder_workspace_bytes<Enc>(obs_dim, n_minibatch) < 0) return EVAC_ERR_INVALID_ARGUMENT;
    return encoder_population_layout<Enc>(obs_dim, n_minibatch, n_learners).total;
}

// A sweep's workspace: the population's, unchanged, then the learners' optimiser values (evac::LearnerSteps as the host fills it)
// on a 256-byte boundary: the last bytes.
constexpr int64_t kStepsTableBytes = (int64_t)sizeof(evac::LearnerSteps);
// The whole body of evac_deepsets_sweep_workspace_bytes / evac_transformer_sweep_workspace_bytes.
template <class Enc>
inline int64_t encoder_sweep_workspace_bytes(int32_t obs_dim, int64_t n_minibatch, int32_t n_learners) {
    const int64_t population = encoder_population_workspace_bytes<Enc>(obs_dim, n_minibatch, n_learners);
    return population < 0 ? population : ws_round_up(population) + ws_round_up(kStepsTableBytes);
}

// The whole body of evac_deepsets_update_population / evac_transformer_update_population; `kernel` is the unit's
// k_adam_set_population / k_adam_tf_population.  With TABLE_UNIT >= 0 the body of encoder_update_sweep below: `hypers` in place
// of use_target_kl / target_kl, refused last, `kernel` the unit's k_adam_set_sweep / k_adam_tf_sweep and TABLE_UNIT what names
// the unit's k_learner_steps_table.
template <class Enc, class Opt, int TABLE_UNIT = -1, class Kernel>
inline int encoder_update_population(Kernel kernel, int32_t n_learners, const evac_mlp_policy_t* policy, const typename Enc::Encoder* encoder,
                                     const evac_mlp_policy_grads_t* params, const typename Enc::Grads* enc_params,
                                     const evac_mlp_policy_grads_t* grads, const typename Enc::Grads* enc_grads,
                                     const evac_mlp_policy_strides_t* param_strides, const typename Opt::EncoderStrides* enc_param_strides,
                                     const evac_mlp_policy_strides_t* grad_strides, const typename Opt::EncoderStrides* enc_grad_strides,
                                     const evac_mlp_policy_strides_t* moment_strides, const typename Opt::EncoderStrides* enc_moment_strides,
                                     int64_t header_stride_bytes, const evac_rpo_loss_config_t* loss_cfg, const evac_adam_config_t* adam_cfg,
                                     const typename Opt::State* state, int64_t batch_size, const float* b_obs, const float* b_actions,
                                     const float* b_logprobs, const float* b_advantages, const float* b_returns, const float* b_values,
                                     int64_t learner_batch_size, int64_t n_minibatch, int32_t n_epochs, const int64_t* perms,
                                     const float* rpo_noise, const uint64_t* seeds, const uint64_t* first_draw_counters,
                                     int32_t use_target_kl, double target_kl, float* stats_out, void* workspace, void* stream,
                                     const evac_learner_hyper_t* hypers = nullptr) {
    constexpr bool kSweep = TABLE_UNIT >= 0;
    static_assert(!kSweep || sizeof(typename Opt::Args) + sizeof(typename Opt::Strides) + sizeof(void*) <= 4096,
                  "the sweep's optimiser kernel: arguments beyond the kernel-argument segment");
    static_assert(sizeof(typename Enc::Args) + 8 + sizeof(void*) + sizeof(typename Enc::LearnerStrides) <= 4096,
                  "the population's encoder kernels: arguments beyond the kernel-argument segment");
    static_assert(sizeof(typename Opt::Args) + sizeof(typename Opt::Strides) <= 4096,
                  "the population's optimiser kernel: arguments beyond the kernel-argument segment");
    // the lone learner's checks of the gradient's arguments (into `s`; its RpoArgs is the population's below) ...
    evac::RpoArgs lone_a;
    typename Enc::Args s;
    if (const int rc = encoder_grad_prepare<Enc>(policy, encoder, loss_cfg, batch_size, b_obs, b_actions, b_logprobs, b_advantages,
                                                 b_returns, b_values, n_minibatch, perms, rpo_noise, 0, grads, enc_grads, stats_out,
                                                 workspace, lone_a, s);
        rc != EVAC_OK)
        return rc;
    // ... the population's of the 13 tensors, the learners and their strides ...
    if (!state) return EVAC_ERR_INVALID_ARGUMENT;
    const evac_adam_state_t linear{state->header, state->exp_avg, state->exp_avg_sq};
    evac::RpoArgs a;
    evac::AdamArgs o;
    evac::LearnerStrides q;
    evac::LearnerDraws d;
    if (const int rc = population_prepare(n_learners, policy, params, grads, param_strides, grad_strides, moment_strides,
                                          header_stride_bytes, loss_cfg, adam_cfg, &linear, batch_size, b_obs, b_actions, b_logprobs,
                                          b_advantages, b_returns, b_values, learner_batch_size, n_minibatch, n_epochs, perms, rpo_noise,
                                          seeds, first_draw_counters, stats_out, workspace, a, o, q, d);
        rc != EVAC_OK)
        return rc;
    // ... the encoder's strides ...
    if (!enc_param_strides || !enc_grad_strides || !enc_moment_strides) return EVAC_ERR_INVALID_ARGUMENT;
    typename Enc::LearnerStrides sq{};
    typename Opt::Strides aq{};
    if (!Opt::strides(*encoder, a.D, n_learners, enc_param_strides, enc_grad_strides, enc_moment_strides, sq, aq))
        return EVAC_ERR_INVALID_ARGUMENT;
    // ... and the lone learner's of the optimiser's tensors (into `qa`; its AdamArgs is the population's above)
    evac::AdamArgs lone_o;
    typename Opt::Args qa;
    if (const int rc = encoder_adam_prepare<Opt>(params, enc_params, grads, enc_grads, state, adam_cfg, policy->obs_dim,
                                                 Opt::dims(*encoder), lone_o, qa);
        rc != EVAC_OK)
        return rc;
    // ... and, of a sweep, the learners' values
    evac::LearnerLoss hl;
    evac::LearnerSteps hs;
    if constexpr (kSweep) {
        if (!learner_hypers_ok(hypers, n_learners)) return EVAC_ERR_INVALID_ARGUMENT;
        learner_values(hypers, n_learners, hl, hs);
    }
    const int64_t S = n_learners;
    const PopulationLayout PL = encoder_population_layout<Enc>(a.D, n_minibatch, S);
    q.ws = PL.slice;                                   // (population_prepare's is the linear learner's slice)
    sq.w1a = q.p[0]; sq.w1c = q.p[7];
    sq.hdr = q.hdr; sq.ws = q.ws; sq.inds = q.inds; sq.stats = q.stats;
    for (int i = 0; i < evac::kAdamTensors; ++i) {
        aq.p[i] = q.p[i]; aq.g[i] = q.g[i]; aq.m[i] = q.m[i];
    }
    aq.hdr = q.hdr; aq.stats = q.stats;
    o.use_target_kl = use_target_kl != 0;
    o.target_kl = target_kl;
    const int dev = device_of(workspace);
    DeviceGuard g(dev);
    if constexpr (kSweep) {                            // (the limit is the launched kernel's own)
        if (evac::sweep_raise_grad_lds(a.D, dev) != EVAC_OK) return EVAC_ERR_HIP;
    } else {
        if (evac::population_raise_grad_lds(a.D, dev) != EVAC_OK) return EVAC_ERR_HIP;
    }
    hipStream_t stream_ = (hipStream_t)stream;
    evac::population_launch_begin(o.hdr, header_stride_bytes, n_learners, stream_);
    char* const common = (char*)workspace;
    evac::LearnerSteps* const table = (evac::LearnerSteps*)(common + ws_round_up(PL.total));
    if constexpr (kSweep)
        hipLaunchKernelGGL(evac::k_learner_steps_table<TABLE_UNIT>, dim3(1), dim3(evac::kStepsTableBlock), 0, stream_, hs, table);
    // (draw counter base 0: the kernels add the learner's first draw counter)
    rpo_update_steps(a, o, learner_batch_size, n_minibatch, n_epochs, perms, rpo_noise, stats_out, 0,
                     [&](const evac::RpoArgs& step, const evac::AdamArgs& adam, uint64_t) {
                         // learner 0's step as the lone update shapes it, then its encoded batch moved into the common one
                         evac::RpoArgs inner = encoder_grad_step<Enc>(step, s);
                         s.Y = (float*)(common + PL.Y);
                         s.act_g = (float*)(common + PL.cols.act); s.lp_g = (float*)(common + PL.cols.lp);
                         s.adv_g = (float*)(common + PL.cols.adv); s.ret_g = (float*)(common + PL.cols.ret);
                         s.val_g = (float*)(common + PL.cols.val); s.ident = (int64_t*)(common + PL.cols.ident);
                         inner.obs = s.Y; inner.actions = s.act_g; inner.logprobs = s.lp_g; inner.adv = s.adv_g; inner.ret = s.ret_g;
                         inner.val = s.val_g; inner.inds = s.ident;
                         inner.B = S * step.M;
                         evac::LearnerStrides qi = q;
                         qi.inds = step.M;                // learner s's index list: s M + m
                         encoder_adam_scalars(adam, qa);
                         const evac::AdamHeader* gate = adam.hdr;
                         const unsigned L = (unsigned)n_learners;
                         const LearnerGrids grid = learner_grids(inner, adam, L);
                         Enc::encode(s, L, stream_, gate, sq);
                         if (inner.norm_adv) evac::population_launch_adv_stats(inner, qi, d, gate, n_learners, stream_);
                         if constexpr (kSweep) {
                             evac::sweep_launch_grad(inner, qi, d, hl, gate, grid.grad, grid.lds, stream_);
                             evac::sweep_launch_finish(inner, qi, d, hl, gate, grid.finish, stream_);
                         } else {
                             evac::population_launch_grad(inner, qi, d, gate, grid.grad, grid.lds, stream_);
                             evac::population_launch_finish(inner, qi, d, gate, grid.finish, stream_);
                         }
                         Enc::backward(s, L, stream_, gate, sq);
                         if constexpr (kSweep) Opt::launch(kernel, qa, L, stream_, aq, (const evac::LearnerSteps*)table);
                         else Opt::launch(kernel, qa, L, stream_, aq);
                     });
    return hipGetLastError() == hipSuccess ? EVAC_OK : EVAC_ERR_HIP;
}

// The whole body of evac_deepsets_update_sweep / evac_transformer_update_sweep: encoder_update_population's checks, step loop and
// launches with every learner's own clip / ent / vf / alpha (the gradient and its finish), lr / max_grad_norm / target_kl (the
// optimiser); one launch more per call, the table's.  `kernel`: the unit's k_adam_set_sweep / k_adam_tf_sweep.
template <class Enc, class Opt, int TABLE_UNIT, class Kernel>
inline int encoder_update_sweep(Kernel kernel, int32_t n_learners, const evac_mlp_policy_t* policy, const typename Enc::Encoder* encoder,
                                const evac_mlp_policy_grads_t* params, const typename Enc::Grads* enc_params,
                                const evac_mlp_policy_grads_t* grads, const typename Enc::Grads* enc_grads,
                                const evac_mlp_policy_strides_t* param_strides, const typename Opt::EncoderStrides* enc_param_strides,
                                const evac_mlp_policy_strides_t* grad_strides, const typename Opt::EncoderStrides* enc_grad_strides,
                                const evac_mlp_policy_strides_t* moment_strides, const typename Opt::EncoderStrides* enc_moment_strides,
                                int64_t header_stride_bytes, const evac_rpo_loss_config_t* loss_cfg, const evac_adam_config_t* adam_cfg,
                                const typename Opt::State* state, int64_t batch_size, const float* b_obs, const float* b_actions,
                                const float* b_logprobs, const float* b_advantages, const float* b_returns, const float* b_values,
                                int64_t learner_batch_size, int64_t n_minibatch, int32_t n_epochs, const int64_t* perms,
                                const float* rpo_noise, const uint64_t* seeds, const uint64_t* first_draw_counters,
                                const evac_learner_hyper_t* hypers, float* stats_out, void* workspace, void* stream) {
    static_assert(TABLE_UNIT >= 0, "a sweep names its unit's k_learner_steps_table");
    return encoder_update_population<Enc, Opt, TABLE_UNIT>(
        kernel, n_learners, policy, encoder, params, enc_params, grads, enc_grads, param_strides, enc_param_strides, grad_strides,
        enc_grad_strides, moment_strides, enc_moment_strides, header_stride_bytes, loss_cfg, adam_cfg, state, batch_size, b_obs, b_actions,
        b_logprobs, b_advantages, b_returns, b_values, learner_batch_size, n_minibatch, n_epochs, perms, rpo_noise, seeds,
        first_draw_counters, 0, 0.0, stats_out, workspace, stream, hypers);
}

}  // namespace
