// Host side of the update of a population of transformer leaders (include/evac.h: evac_transformer_population_workspace_bytes,
// evac_transformer_update_population; kernels in evac_transformer_population_train.h and evac_transformer_train.h and, for the
// three launches in the middle of a step, evac_population.h's through evac_population_host.h's launch functions).  The update is
// evac_transformer_update's checks (encoder_grad_prepare, tf_adam_prepare) and evac_rpo_update_population's (population_prepare)
// over one step loop (rpo_update_steps), with the learner as one more grid dimension of each launch:
// evac_deepsets_update_population's body with TfGrad where SetGrad stood.  Every refusal before the first HIP call, no device
// allocation, no synchronisation.
#include <hip/hip_runtime.h>

#include <cstddef>
#include <cstdint>

#include "evac_transformer_population_train.h"
#include "evac_transformer_adam_host.h"
#include "evac_population_host.h"

static_assert(sizeof(evac::TfgArgs) + 8 + sizeof(void*) + sizeof(evac::TfgLearnerStrides) <= 4096,
              "the population's encoder kernels: arguments beyond the kernel-argument segment");
static_assert(sizeof(evac::RpoArgs) + sizeof(evac::LearnerStrides) + sizeof(evac::LearnerDraws) + sizeof(void*) <= 4096,
              "the gradient kernels' arguments must fit the kernel-argument segment");
static_assert(kWsAlign % kSliceAlign == 0, "slices of whole 256-byte parts: no two learners share a 128-byte line");

namespace {

// The workspace: S slices of the lone learner's (TfGrad::layout: every part on a 256-byte boundary, its Y and gathered columns
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
    L.slice = ws_round_up(TfGrad::layout(D, M).total);
    WsCursor c{L.slice * S};
    L.Y = c.take(S * M * D * (int64_t)sizeof(float));
    L.cols = take_gathered(c, S * M);
    L.total = c.o;
    return L;
}

// evac_transformer_strides_t's strides of the blocks in use into [block][tensor] (the others stay 0: never looked at)
void copy_block_strides(const evac_transformer_strides_t* st, int num_blocks, int64_t (*dst)[evac::kTfgTensors]) {
    for (int b = 0; b < num_blocks; ++b)
        for (int i = 0; i < evac::kTfgTensors; ++i) dst[b][i] = (&st->blocks[b].wq)[i];
}

}  // namespace

extern "C" {

int64_t evac_transformer_population_workspace_bytes(int32_t obs_dim, int64_t n_minibatch, int32_t n_learners) {
    if (n_learners < 1 || n_learners > EVAC_MAX_LEARNERS) return EVAC_ERR_INVALID_ARGUMENT;
    if (encoder_workspace_bytes<TfGrad>(obs_dim, n_minibatch) < 0) return EVAC_ERR_INVALID_ARGUMENT;
    return population_layout(obs_dim, n_minibatch, n_learners).total;
}

int evac_transformer_update_population(int32_t n_learners, const evac_mlp_policy_t* policy, const evac_transformer_t* encoder,
                                       const evac_mlp_policy_grads_t* params, const evac_transformer_grads_t* enc_params,
                                       const evac_mlp_policy_grads_t* grads, const evac_transformer_grads_t* enc_grads,
                                       const evac_mlp_policy_strides_t* param_strides, const evac_transformer_strides_t* enc_param_strides,
                                       const evac_mlp_policy_strides_t* grad_strides, const evac_transformer_strides_t* enc_grad_strides,
                                       const evac_mlp_policy_strides_t* moment_strides, const evac_transformer_strides_t* enc_moment_strides,
                                       int64_t header_stride_bytes, const evac_rpo_loss_config_t* loss_cfg,
                                       const evac_adam_config_t* adam_cfg, const evac_transformer_adam_state_t* state, int64_t batch_size,
                                       const float* b_obs, const float* b_actions, const float* b_logprobs, const float* b_advantages,
                                       const float* b_returns, const float* b_values, int64_t learner_batch_size, int64_t n_minibatch,
                                       int32_t n_epochs, const int64_t* perms, const float* rpo_noise, const uint64_t* seeds,
                                       const uint64_t* first_draw_counters, int32_t use_target_kl, double target_kl, float* stats_out,
                                       void* workspace, void* stream) {
    // the lone learner's checks of the gradient's arguments (into `s`; its RpoArgs is the population's below) ...
    evac::RpoArgs lone_a;
    evac::TfgArgs s;
    if (const int rc = encoder_grad_prepare<TfGrad>(policy, encoder, loss_cfg, batch_size, b_obs, b_actions, b_logprobs, b_advantages,
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
    const int dm = encoder->elem_dim, nb = encoder->num_blocks;
    if (!transformer_strides_ok(enc_param_strides, dm, nb, n_learners) || !transformer_strides_ok(enc_grad_strides, dm, nb, n_learners) ||
        !transformer_strides_ok(enc_moment_strides, dm, nb, n_learners))
        return EVAC_ERR_INVALID_ARGUMENT;
    // ... and the lone learner's of the optimiser's 13 + 16 num_blocks tensors (into `qa`; its AdamArgs is the population's above)
    evac::AdamArgs lone_o;
    evac::TfAdamArgs qa;
    if (const int rc = tf_adam_prepare(params, enc_params, grads, enc_grads, state, adam_cfg, policy->obs_dim, dm, nb, lone_o, qa);
        rc != EVAC_OK)
        return rc;
    const int64_t S = n_learners;
    const PopulationLayout PL = population_layout(a.D, n_minibatch, S);
    q.ws = PL.slice;                                   // (population_prepare's is the linear learner's slice)
    evac::TfgLearnerStrides sq{};
    evac::TfAdamStrides aq{};
    int64_t enc_m[evac::kTfgMaxBlocks][evac::kTfgTensors] = {};
    copy_block_strides(enc_param_strides, nb, sq.p);
    copy_block_strides(enc_grad_strides, nb, sq.g);
    copy_block_strides(enc_moment_strides, nb, enc_m);
    sq.w1a = q.p[0]; sq.w1c = q.p[7];
    sq.hdr = q.hdr; sq.ws = q.ws; sq.inds = q.inds; sq.stats = q.stats;
    for (int i = 0; i < evac::kAdamTensors; ++i) {
        aq.p[i] = q.p[i]; aq.g[i] = q.g[i]; aq.m[i] = q.m[i];
    }
    for (int b = 0; b < nb; ++b)
        for (int i = 0; i < evac::kTfgTensors; ++i) {
            const int t = evac::kAdamTensors + b * evac::kTfAdamBlockTensors + i;
            aq.p[t] = sq.p[b][i]; aq.g[t] = sq.g[b][i]; aq.m[t] = enc_m[b][i];
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
                         // learner 0's step as evac_transformer_update shapes it, then its encoded batch moved into the common one
                         evac::RpoArgs inner = encoder_grad_step<TfGrad>(step, s);
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
                         // TfGrad::launch's grids, the learner as y
                         const int64_t M = s.M;
                         const int64_t enc_wgs = (M + evac::kTfgEncodeWaves - 1) / evac::kTfgEncodeWaves;
                         const int64_t tiles = (M + evac::kTfgTile - 1) / evac::kTfgTile;
                         const dim3 block(evac::kTfgEncodeBlock);
                         hipLaunchKernelGGL((evac::k_tf_encode<const evac::AdamHeader*, evac::TfgLearnerStrides>),
                                            dim3((unsigned)(enc_wgs > evac::kTfgEncodeMaxWgs ? evac::kTfgEncodeMaxWgs : enc_wgs), L), block,
                                            0, stream_, s, gate, sq);
                         if (inner.norm_adv) evac::population_launch_adv_stats(inner, qi, d, gate, n_learners, stream_);
                         evac::population_launch_grad(inner, qi, d, gate, grid.grad, grid.lds, stream_);
                         evac::population_launch_finish(inner, qi, d, gate, grid.finish, stream_);
                         hipLaunchKernelGGL((evac::k_tf_dy<const evac::AdamHeader*, evac::TfgLearnerStrides>),
                                            dim3((unsigned)(tiles > 65536 ? 65536 : tiles), L), block, 0, stream_, s, gate, sq);
                         for (int b = s.nb - 1; b >= 0; --b)
                             hipLaunchKernelGGL((evac::k_tf_backward<const evac::AdamHeader*, evac::TfgLearnerStrides>),
                                                dim3((unsigned)s.P, L), dim3(evac::kTfgBlock), 0, stream_, s, b, gate, sq);
                         hipLaunchKernelGGL((evac::k_tf_finish<const evac::AdamHeader*, evac::TfgLearnerStrides>),
                                            dim3((unsigned)(s.nb * evac::kTfgFinishWgs), L), block, 0, stream_, s, gate, sq);
                         tf_adam_launch(evac::k_adam_tf_population, qa, L, stream_, aq);
                     });
    return hipGetLastError() == hipSuccess ? EVAC_OK : EVAC_ERR_HIP;
}

}  // extern "C"
