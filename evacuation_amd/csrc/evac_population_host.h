// Host side of the population's update, the part its two translation units share (evac_population_api.hip: one configuration;
// evac_sweep_api.hip: a configuration per learner; evac_deepsets_population_api.hip: behind a set encoder): the checks and the
// learners' strides, a step's grids, and the launches of evac_population_api.hip that the other units reuse (no hyperparameter
// enters them), reached through plain host functions so that evac_population.h's kernels are defined in one translation unit alone.
#pragma once

#include "evac_learner.h"
#include "evac_train_host.h"

namespace evac {
// k_population_begin and k_population_adv_stats on `stream` (evac_population_api.hip)
void population_launch_begin(AdamHeader* hdr, int64_t header_stride_bytes, int n_learners, hipStream_t stream);
void population_launch_adv_stats(const RpoArgs& a, const LearnerStrides& q, const LearnerDraws& d, const AdamHeader* gate,
                                 int n_learners, hipStream_t stream);
// k_population_grad and k_population_finish on `stream`, for the population of deep-sets leaders (evac_deepsets_population_api.hip:
// the same launches on the learners' encoded batch), and the raising of k_population_grad's dynamic-LDS limit (rpo_raise_lds)
void population_launch_grad(const RpoArgs& a, const LearnerStrides& q, const LearnerDraws& d, const AdamHeader* gate, dim3 grid,
                            size_t lds, hipStream_t stream);
void population_launch_finish(const RpoArgs& a, const LearnerStrides& q, const LearnerDraws& d, const AdamHeader* gate, dim3 grid,
                              hipStream_t stream);
int population_raise_grad_lds(int D, int dev);
}  // namespace evac

namespace {
constexpr int64_t kSliceAlign = 128;            // a learner's workspace slice starts on a cache line of its own

inline int64_t slice_bytes(int32_t obs_dim, int64_t n_minibatch) {
    const int64_t one = evac_rpo_workspace_bytes(obs_dim, n_minibatch);
    return one < 0 ? one : (one + kSliceAlign - 1) / kSliceAlign * kSliceAlign;
}
// The grids of a step's gradient, finishing and optimiser launches for L learners (the one-learner kernels' with the learner as
// one more dimension) and the gradient kernel's dynamic LDS
struct LearnerGrids {
    dim3 grad, finish, optimizer;
    size_t lds;
};
inline LearnerGrids learner_grids(const evac::RpoArgs& a, const evac::AdamArgs& o, unsigned L) {
    const int tiles = (a.D + evac::kW1Tile - 1) / evac::kW1Tile, n = o.end[evac::kAdamTensors - 1];
    return {dim3((unsigned)a.P, 2u, L), dim3((unsigned)(2 * evac::kFinishCombineWgs + 2 * tiles * a.S), L),
            dim3((unsigned)((n + evac::kAdamBlock - 1) / evac::kAdamBlock), L), evac::rpo_grad_lds_floats(a.D) * sizeof(float)};
}
// What evac_rpo_update_population checks and sets up: learner 0's argument structs, the learners' strides and draws.
inline int population_prepare(int32_t n_learners, const evac_mlp_policy_t* policy, const evac_mlp_policy_grads_t* params,
                              const evac_mlp_policy_grads_t* grads, const evac_mlp_policy_strides_t* param_strides,
                              const evac_mlp_policy_strides_t* grad_strides, const evac_mlp_policy_strides_t* moment_strides,
                              int64_t header_stride_bytes, const evac_rpo_loss_config_t* loss_cfg, const evac_adam_config_t* adam_cfg,
                              const evac_adam_state_t* state, int64_t batch_size, const float* b_obs, const float* b_actions,
                              const float* b_logprobs, const float* b_advantages, const float* b_returns, const float* b_values,
                              int64_t learner_batch_size, int64_t n_minibatch, int32_t n_epochs, const int64_t* perms,
                              const float* rpo_noise, const uint64_t* seeds, const uint64_t* first_draw_counters, float* stats_out,
                              void* workspace, evac::RpoArgs& a, evac::AdamArgs& o, evac::LearnerStrides& q, evac::LearnerDraws& d) {
    if (n_learners < 1 || n_learners > EVAC_MAX_LEARNERS || n_epochs < 1 || learner_batch_size < 1) return EVAC_ERR_INVALID_ARGUMENT;
    if (!param_strides || !grad_strides || !moment_strides || !seeds || !first_draw_counters) return EVAC_ERR_INVALID_ARGUMENT;
    int rc = rpo_prepare(policy, loss_cfg, batch_size, b_obs, b_actions, b_logprobs, b_advantages, b_returns, b_values, n_minibatch,
                         perms, rpo_noise, 0, grads, stats_out, workspace, a);
    if (rc != EVAC_OK) return rc;
    rc = adam_prepare(params, grads, state, adam_cfg, policy->obs_dim, o);
    if (rc != EVAC_OK) return rc;
    q = evac::LearnerStrides{};
    if (!mlp_strides_ok(param_strides, a.D, n_learners, q.p) || !mlp_strides_ok(grad_strides, a.D, n_learners, q.g) ||
        !mlp_strides_ok(moment_strides, a.D, n_learners, q.m))
        return EVAC_ERR_INVALID_ARGUMENT;
    if (n_learners > 1 && (header_stride_bytes < (int64_t)sizeof(evac::AdamHeader) || (header_stride_bytes & 7) != 0))
        return EVAC_ERR_INVALID_ARGUMENT;
    const int64_t B = learner_batch_size, M = n_minibatch;
    const int64_t steps = rpo_steps_per_epoch(B, M, a.norm_adv ? 2 : 1) * n_epochs;     // of one learner, in the whole call
    q.hdr = header_stride_bytes;
    q.ws = slice_bytes(a.D, M);
    q.inds = (int64_t)n_epochs * B;
    q.stats = steps * 8;
    q.noise = steps * M * 2;
    d = evac::LearnerDraws{};
    for (int s = 0; s < n_learners; ++s) {
        d.seed[s] = seeds[s];
        d.first_counter[s] = first_draw_counters[s];
    }
    o.gated = 1;
    return EVAC_OK;
}
}  // namespace
