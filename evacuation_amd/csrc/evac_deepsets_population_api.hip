// Host side of a population of deep-sets leaders (include/evac.h: evac_policy_rollout_population_deepsets,
// evac_deepsets_population_workspace_bytes, evac_deepsets_update_population; kernels in evac_deepsets_population.h and, for the
// three launches in the middle of a step, evac_population.h's through evac_population_host.h's launch functions).  Collection is
// evac_handle_host.h's encoder_rollout with the learners' shares; the update is evac_deepsets_update's checks (encoder_grad_prepare,
// set_adam_prepare) and evac_rpo_update_population's (population_prepare) over one step loop (rpo_update_steps), with the learner
// as one more grid dimension of each launch.  Every refusal before the first HIP call, no device allocation, no synchronisation.
#include <hip/hip_runtime.h>

#include <cstddef>
#include <cstdint>
#include <string>

#define EVAC_TEMPLATE_KERNELS_ONLY      // (evac_device.h: its plain kernels live in evac_api.hip)
#include "evac_deepsets_population.h"
#include "evac_deepsets_adam_host.h"
#include "evac_deepsets_host.h"
#include "evac_handle_host.h"
#include "evac_host.h"
#include "evac_population_host.h"

static_assert(sizeof(evac::Params) + 8 + sizeof(evac::PolicyArgs) + sizeof(evac::NormArgs) + sizeof(evac::PopulationArgs) +
                      sizeof(evac::DeepSetsArgs) + sizeof(evac::DeepSetsStrides) <= 4096,
              "k_collect_population_deepsets: arguments beyond the kernel-argument segment");
static_assert(sizeof(evac::SetArgs) + sizeof(void*) + sizeof(evac::SetLearnerStrides) <= 4096,
              "the population's encoder kernels: arguments beyond the kernel-argument segment");
static_assert(sizeof(evac::SetAdamArgs) + sizeof(evac::SetAdamStrides) <= 4096,
              "k_adam_set_population: arguments beyond the kernel-argument segment");
static_assert(sizeof(evac::RpoArgs) + sizeof(evac::LearnerStrides) + sizeof(evac::LearnerDraws) + sizeof(void*) <= 4096,
              "the gradient kernels' arguments must fit the kernel-argument segment");
static_assert(kWsAlign % kSliceAlign == 0, "slices of whole 256-byte parts: no two learners share a 128-byte line");

namespace {

// evac_handle_host.h's trait of an encoder, for the population's collection entry (the lone kernels are evac_deepsets_api.hip's)
struct DeepSetsPopulationEncoder : DeepSetsEncoderHost {
    static constexpr const char* kRollout = "evac_policy_rollout_population_deepsets";
};
// ... and its learners: their shares of the handle's envs and the strides of their 19 tensors (evac_deepsets_host.h), the launch
struct DeepSetsLearners : DeepSetsLearnerShares {
    void launch(const evac_host::HandleView& v, int n_steps, const evac::PolicyArgs& a, const evac::NormArgs& na,
                const evac::DeepSetsArgs& ea, hipStream_t S) const {
        const auto fn = EVAC_PICK_BOOL2(evac::k_collect_population_deepsets, na.state != nullptr, v.default_cfg);
        hipLaunchKernelGGL(fn, dim3((unsigned)(n_learners * q.wgs)), dim3(evac::PolicyFamily::kBlock), 0, S, v.p, n_steps, a, na, q, ea, dq);
    }
};

// The workspace: S slices of the lone learner's (SetGrad::layout: every part on a 256-byte boundary, its Y and gathered columns
// left unused), then what the actor-critic's kernels read as one common batch of S x M rows: Y | the gathered actions,
// log-probabilities, advantages, returns, values | the index lists.  A step of m <= M samples packs the learners' rows densely:
// learner s's begin s x m rows into each part.
struct PopulationLayout {
    int64_t slice, Y;
    GatheredLayout cols;
    int64_t total;
};
PopulationLayout population_layout(int32_t D, int64_t M, int64_t S) {
    PopulationLayout L;
    L.slice = ws_round_up(SetGrad::layout(D, M).total);
    WsCursor c{L.slice * S};
    L.Y = c.take(S * M * D * (int64_t)sizeof(float));
    L.cols = take_gathered(c, S * M);
    L.total = c.o;
    return L;
}

}  // namespace

extern "C" {

int evac_policy_rollout_population_deepsets(evac_handle_t h, int32_t n_learners, const evac_mlp_policy_t* policy,
                                            const evac_mlp_policy_strides_t* strides, const evac_deepsets_t* encoder,
                                            const evac_deepsets_strides_t* enc_strides, int32_t n_steps, float* next_obs,
                                            float* next_done, float* obs_out, float* actions_out, float* logprob_out, float* value_out,
                                            float* reward_out, float* done_out, float* next_value_out, evac_episode_stats_t* final_stats,
                                            double* norm_state, float gamma, float obs_clip, float reward_clip, float epsilon,
                                            void* stream) {
    if (!strides || !enc_strides) {
        evac_host::HandleView v;
        if (const int rc = evac_host::handle_begin(h, DeepSetsPopulationEncoder::kRollout, &v); rc != EVAC_OK) return rc;
        return evac_host::handle_fail(h, EVAC_ERR_INVALID_ARGUMENT,
                                      std::string(DeepSetsPopulationEncoder::kRollout) + ": strides / enc_strides is NULL");
    }
    return encoder_rollout<DeepSetsPopulationEncoder>(h, n_steps, policy,
                                                      collect_outputs(next_obs, next_done, obs_out, actions_out, logprob_out, value_out,
                                                                      reward_out, done_out, next_value_out, final_stats),
                                                      evac::NormArgs{norm_state, gamma, obs_clip, reward_clip, epsilon}, encoder, stream,
                                                      DeepSetsLearners{{n_learners, strides, enc_strides}});
}

int64_t evac_deepsets_population_workspace_bytes(int32_t obs_dim, int64_t n_minibatch, int32_t n_learners) {
    if (n_learners < 1 || n_learners > EVAC_MAX_LEARNERS) return EVAC_ERR_INVALID_ARGUMENT;
    if (encoder_workspace_bytes<SetGrad>(obs_dim, n_minibatch) < 0) return EVAC_ERR_INVALID_ARGUMENT;
    return population_layout(obs_dim, n_minibatch, n_learners).total;
}

int evac_deepsets_update_population(int32_t n_learners, const evac_mlp_policy_t* policy, const evac_deepsets_t* encoder,
                                    const evac_mlp_policy_grads_t* params, const evac_deepsets_grads_t* enc_params,
                                    const evac_mlp_policy_grads_t* grads, const evac_deepsets_grads_t* enc_grads,
                                    const evac_mlp_policy_strides_t* param_strides, const evac_deepsets_strides_t* enc_param_strides,
                                    const evac_mlp_policy_strides_t* grad_strides, const evac_deepsets_strides_t* enc_grad_strides,
                                    const evac_mlp_policy_strides_t* moment_strides, const evac_deepsets_strides_t* enc_moment_strides,
                                    int64_t header_stride_bytes, const evac_rpo_loss_config_t* loss_cfg,
                                    const evac_adam_config_t* adam_cfg, const evac_deepsets_adam_state_t* state, int64_t batch_size,
                                    const float* b_obs, const float* b_actions, const float* b_logprobs, const float* b_advantages,
                                    const float* b_returns, const float* b_values, int64_t learner_batch_size, int64_t n_minibatch,
                                    int32_t n_epochs, const int64_t* perms, const float* rpo_noise, const uint64_t* seeds,
                                    const uint64_t* first_draw_counters, int32_t use_target_kl, double target_kl, float* stats_out,
                                    void* workspace, void* stream) {
    // the lone learner's checks of the gradient's arguments (into `s`; its RpoArgs is the population's below) ...
    evac::RpoArgs lone_a;
    evac::SetArgs s;
    if (const int rc = encoder_grad_prepare<SetGrad>(policy, encoder, loss_cfg, batch_size, b_obs, b_actions, b_logprobs, b_advantages,
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
    evac::SetLearnerStrides sq{};
    evac::SetAdamStrides aq{};
    const int ed = encoder->set_elem_dim;
    if (!deepsets_strides_ok(enc_param_strides, a.D, ed, n_learners, sq.p) || !deepsets_strides_ok(enc_grad_strides, a.D, ed, n_learners, sq.g) ||
        !deepsets_strides_ok(enc_moment_strides, a.D, ed, n_learners, aq.m + evac::kAdamTensors))
        return EVAC_ERR_INVALID_ARGUMENT;
    // ... and the lone learner's of the optimiser's 19 tensors (into `qa`; its AdamArgs is the population's above)
    evac::AdamArgs lone_o;
    evac::SetAdamArgs qa;
    if (const int rc = set_adam_prepare(params, enc_params, grads, enc_grads, state, adam_cfg, policy->obs_dim, encoder->set_elem_dim,
                                        lone_o, qa);
        rc != EVAC_OK)
        return rc;
    const int64_t S = n_learners;
    const PopulationLayout PL = population_layout(a.D, n_minibatch, S);
    q.ws = PL.slice;                                   // (population_prepare's is the linear learner's slice)
    sq.w1a = q.p[0]; sq.w1c = q.p[7];
    sq.hdr = q.hdr; sq.ws = q.ws; sq.inds = q.inds; sq.stats = q.stats;
    for (int i = 0; i < evac::kAdamTensors; ++i) {
        aq.p[i] = q.p[i]; aq.g[i] = q.g[i]; aq.m[i] = q.m[i];
    }
    for (int i = 0; i < 6; ++i) {
        aq.p[evac::kAdamTensors + i] = sq.p[i]; aq.g[evac::kAdamTensors + i] = sq.g[i];
    }
    aq.hdr = q.hdr; aq.stats = q.stats;
    o.use_target_kl = use_target_kl != 0;
    o.target_kl = target_kl;
    const int dev = device_of(workspace);
    DeviceGuard g(dev);
    if (evac::population_raise_grad_lds(a.D, dev) != EVAC_OK) return EVAC_ERR_HIP;
    hipStream_t stream_ = (hipStream_t)stream;
    evac::population_launch_begin(o.hdr, header_stride_bytes, n_learners, stream_);
    char* const common = (char*)workspace;
    // (draw counter base 0: the kernels add the learner's first draw counter)
    rpo_update_steps(a, o, learner_batch_size, n_minibatch, n_epochs, perms, rpo_noise, stats_out, 0,
                     [&](const evac::RpoArgs& step, const evac::AdamArgs& adam, uint64_t) {
                         // learner 0's step as evac_deepsets_update shapes it, then its encoded batch moved into the common one
                         evac::RpoArgs inner = encoder_grad_step<SetGrad>(step, s);
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
                         const int64_t M = s.M;
                         const int64_t enc_wgs = (M + evac::kSetWaves - 1) / evac::kSetWaves;
                         const dim3 block(evac::kSetBlock);
                         hipLaunchKernelGGL((evac::k_set_encode<const evac::AdamHeader*, evac::SetLearnerStrides>),
                                            dim3((unsigned)(enc_wgs > evac::kSetEncodeMaxWgs ? evac::kSetEncodeMaxWgs : enc_wgs), L), block, 0,
                                            stream_, s, gate, sq);
                         if (inner.norm_adv) evac::population_launch_adv_stats(inner, qi, d, gate, n_learners, stream_);
                         evac::population_launch_grad(inner, qi, d, gate, grid.grad, grid.lds, stream_);
                         evac::population_launch_finish(inner, qi, d, gate, grid.finish, stream_);
                         hipLaunchKernelGGL((evac::k_set_backward<const evac::AdamHeader*, evac::SetLearnerStrides>), dim3((unsigned)s.P, L),
                                            block, 0, stream_, s, gate, sq);
                         const int rtiles = (s.D + evac::kSetRTile - 1) / evac::kSetRTile;
                         hipLaunchKernelGGL((evac::k_set_finish<const evac::AdamHeader*, evac::SetLearnerStrides>),
                                            dim3((unsigned)(rtiles * s.Sr + 1), L), block, 0, stream_, s, gate, sq);
                         hipLaunchKernelGGL(evac::k_adam_set_population, dim3((unsigned)qa.wg_end[evac::kSetAdamTensors - 1], L),
                                            dim3(evac::kAdamBlock), 0, stream_, qa, aq);
                     });
    return hipGetLastError() == hipSuccess ? EVAC_OK : EVAC_ERR_HIP;
}

}  // extern "C"
