// Host side of the trainer's update, the part its translation units share (evac_train_api.hip: one learner;
// evac_population_api.hip: a population; evac_sweep_api.hip: ... with a configuration per learner; evac_deepsets_train_api.hip:
// the gradient behind a set encoder; evac_deepsets_update_api.hip: its optimiser step and whole update;
// evac_transformer_train_api.hip: the gradient behind an attention encoder; evac_transformer_update_api.hip: its optimiser step
// and whole update -- what those four share beyond this file is in evac_encoder_train_host.h; evac_deepsets_population_api.hip:
// a population of deep-sets leaders): what the entries check of
// their arguments, the kernels' argument structs, the walk over an update call's minibatch steps, the raising of a gradient
// kernel's dynamic-LDS limit, and the launches of one minibatch's gradient.
#pragma once

#include <hip/hip_runtime.h>

#include <cmath>
#include <cstddef>
#include <cstdint>
#include <mutex>

#include "evac_host.h"
#include "evac_train.h"

namespace {

// What evac_rpo_minibatch_grad checks and sets up, for every entry that runs the gradient of a minibatch.
inline int rpo_prepare(const evac_mlp_policy_t* policy, const evac_rpo_loss_config_t* cfg, int64_t batch_size, const float* b_obs,
                const float* b_actions, const float* b_logprobs, const float* b_advantages, const float* b_returns,
                const float* b_values, int64_t n_minibatch, const int64_t* mb_inds, const float* rpo_noise, uint64_t seed,
                const evac_mlp_policy_grads_t* grads_out, float* stats_out, void* workspace, evac::RpoArgs& a) {
    if (!policy || !cfg || !b_obs || !b_actions || !b_logprobs || !b_advantages || !b_returns || !b_values || !mb_inds || !grads_out ||
        !stats_out || !workspace)
        return EVAC_ERR_INVALID_ARGUMENT;
    const evac_mlp_policy_t& P = *policy;
    const evac_mlp_policy_grads_t& G = *grads_out;
    if (!mlp_all_set(P) || !mlp_all_set(G)) return EVAC_ERR_INVALID_ARGUMENT;
    if (P.hidden != evac::kTrainHidden || P.obs_dim < 1 || P.obs_dim > evac::kTrainMaxObs)
        return EVAC_ERR_INVALID_ARGUMENT;
    if (batch_size < 1 || n_minibatch < 1 || n_minibatch >= (int64_t)1 << 31 || (cfg->norm_adv && n_minibatch < 2))
        return EVAC_ERR_INVALID_ARGUMENT;              // (the unbiased std of one sample does not exist)
    if (((uintptr_t)workspace & 15u) != 0) return EVAC_ERR_INVALID_ARGUMENT;
    a = evac::RpoArgs{};
    const float* const* p = mlp_tensors(P);            // (w1 b1 w2 b2 w3 b3 of the actor, logstd, the same six of the critic)
    float* const* g = mlp_tensors(G);
    for (int n = 0; n < 2; ++n) {
        const int o = 7 * n;
        a.net[n] = evac::RpoNet{p[o], p[o + 1], p[o + 2], p[o + 3], p[o + 4], p[o + 5], g[o], g[o + 1], g[o + 2], g[o + 3], g[o + 4], g[o + 5]};
    }
    a.logstd = p[6];
    a.glogstd = g[6];
    a.obs = b_obs; a.actions = b_actions; a.logprobs = b_logprobs; a.adv = b_advantages; a.ret = b_returns; a.val = b_values;
    a.inds = mb_inds;
    a.noise = rpo_noise;
    a.stats = stats_out;
    a.ws = (char*)workspace;
    a.B = batch_size;
    a.clip = cfg->clip_coef; a.ent = cfg->ent_coef; a.vf = cfg->vf_coef; a.alpha = cfg->rpo_alpha;
    a.norm_adv = cfg->norm_adv != 0;
    a.clip_vloss = cfg->clip_vloss != 0;
    a.D = P.obs_dim;
    a.seed_lo = (uint32_t)seed; a.seed_hi = (uint32_t)(seed >> 32);
    return EVAC_OK;
}
// the fields that depend on the minibatch's size and on the draw
inline void rpo_shape(evac::RpoArgs& a, int64_t n_minibatch, uint64_t draw_counter) {
    a.M = (int)n_minibatch;
    const int p0 = evac::rpo_parts_upper(n_minibatch);
    a.chunk = (int)((n_minibatch + p0 - 1) / p0);
    a.P = (int)((n_minibatch + a.chunk - 1) / a.chunk);            // every workgroup has samples (P <= p0: the workspace's bound)
    a.S = evac::rpo_w1_segments(a.D, n_minibatch);
    a.ctr_lo = (uint32_t)draw_counter; a.ctr_hi = (uint32_t)(draw_counter >> 32);
}
// What evac_adam_step checks and sets up.  (!(x > 0) also refuses a NaN.)
inline int adam_prepare(const evac_mlp_policy_grads_t* params, const evac_mlp_policy_grads_t* grads, const evac_adam_state_t* state,
                 const evac_adam_config_t* cfg, int32_t obs_dim, evac::AdamArgs& a) {
    if (!params || !grads || !state || !cfg || !state->header) return EVAC_ERR_INVALID_ARGUMENT;
    if (obs_dim < 1 || obs_dim > evac::kTrainMaxObs) return EVAC_ERR_INVALID_ARGUMENT;
    if (((uintptr_t)state->header & 7u) != 0) return EVAC_ERR_INVALID_ARGUMENT;
    if (!std::isfinite(cfg->lr) || !(cfg->beta1 >= 0.0 && cfg->beta1 < 1.0) || !(cfg->beta2 >= 0.0 && cfg->beta2 < 1.0) ||
        !(cfg->eps > 0.0) || !(cfg->max_grad_norm > 0.0))
        return EVAC_ERR_INVALID_ARGUMENT;
    const evac_mlp_policy_grads_t* sets[4] = {params, grads, &state->exp_avg, &state->exp_avg_sq};
    float** dst[4] = {a.p, a.g, a.m, a.v};
    for (int k = 0; k < 4; ++k) {
        if (!mlp_all_set(*sets[k])) return EVAC_ERR_INVALID_ARGUMENT;
        for (int i = 0; i < evac::kAdamTensors; ++i) dst[k][i] = mlp_tensors(*sets[k])[i];
    }
    const MlpSizes sizes = mlp_sizes(obs_dim);
    int end = 0;
    for (int i = 0; i < evac::kAdamTensors; ++i) a.end[i] = (end += (int)sizes.n[i]);
    a.hdr = (evac::AdamHeader*)state->header;
    a.sumsq = nullptr;
    a.stats = nullptr;
    a.lr = cfg->lr; a.beta1 = cfg->beta1; a.beta2 = cfg->beta2; a.target_kl = 0.0;
    a.max_norm = (float)cfg->max_grad_norm;
    a.w = (float)(1.0 - cfg->beta1); a.b2 = (float)cfg->beta2; a.u = (float)(1.0 - cfg->beta2); a.eps = (float)cfg->eps;
    a.gated = a.epoch_last = a.use_target_kl = 0;
    return EVAC_OK;
}
static_assert(evac::kAdamTensors == kMlpTensors, "the optimiser walks the 13 tensors of evac_mlp_policy_grads_t");
static_assert(evac::kTrainHidden == kMlpHidden, "mlp_sizes: the tensors of the width the trainer's kernels take");

// The minibatch steps of an update call over a (learner's) batch of B samples: for every epoch the starts 0, M, 2M .., without a
// tail shorter than `least` (as RPOTrainer.update() skips it).  step(epoch, start, m, epoch_last, k): m samples from `start`,
// `epoch_last` when no step of this epoch follows, k the step's number in the call.  Returns the number of steps.
template <class Step>
inline uint64_t rpo_walk_steps(int64_t B, int64_t M, int32_t n_epochs, int64_t least, Step&& step) {
    uint64_t k = 0;
    for (int32_t ep = 0; ep < n_epochs; ++ep) {
        for (int64_t start = 0; start < B; start += M) {
            const int64_t m = B - start < M ? B - start : M;
            if (m < least) continue;
            const int64_t next = start + M, m_next = next >= B ? 0 : (B - next < M ? B - next : M);
            step(ep, start, m, m_next < least, k);
            ++k;
        }
    }
    return k;
}
// ... of one epoch, counted alone (population_prepare: the stride of a learner's statistics and noise rows)
inline int64_t rpo_steps_per_epoch(int64_t B, int64_t M, int64_t least) {
    return (int64_t)rpo_walk_steps(B, M, 1, least, [](int32_t, int64_t, int64_t, bool, uint64_t) {});
}
// The step loop of evac_rpo_update and of the population's two entries: `a` and `o` as the prepare functions left them, set for
// step k (its index list, noise row, statistics row, shape, draw counter `counter_base` + k, and whether it ends an epoch), then
// launch(step k's RpoArgs, its AdamArgs, k), which enqueues the step's kernels.  Nothing here calls HIP or allocates.
template <class Launch>
inline void rpo_update_steps(evac::RpoArgs& a, evac::AdamArgs& o, int64_t B, int64_t M, int32_t n_epochs, const int64_t* perms,
                             const float* rpo_noise, float* stats_out, uint64_t counter_base, Launch&& launch) {
    rpo_walk_steps(B, M, n_epochs, a.norm_adv ? 2 : 1, [&](int32_t ep, int64_t start, int64_t m, bool epoch_last, uint64_t k) {
        a.inds = perms + (int64_t)ep * B + start;
        a.noise = rpo_noise ? rpo_noise + k * (uint64_t)M * 2u : nullptr;
        a.stats = stats_out + k * 8u;
        rpo_shape(a, m, counter_base + k);
        o.sumsq = a.stats + 7;
        o.stats = a.stats;
        o.epoch_last = epoch_last;
        launch(a, o, k);
    });
}

// Wide observations: a gradient kernel needs more dynamic LDS than the default limit.  Once per device and kernel: the flags
// belong to the instantiation, that is to `Kernel`'s address.
template <auto Kernel>
inline int rpo_raise_lds(int D, int dev) {
    if (evac::rpo_grad_lds_floats(D) * sizeof(float) <= 64 * 1024) return EVAC_OK;
    static std::mutex mu;
    static bool raised[64] = {};
    std::lock_guard<std::mutex> lock(mu);
    const int slot = dev >= 0 && dev < 64 ? dev : 0;
    if (!raised[slot]) {
        const size_t most = evac::rpo_grad_lds_floats(evac::kTrainMaxObs) * sizeof(float);
        if (hipFuncSetAttribute((const void*)Kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)most) != hipSuccess) {
            (void)hipGetLastError();
            return EVAC_ERR_HIP;
        }
        raised[slot] = true;
    }
    return EVAC_OK;
}

// The launches of one minibatch's gradient.  `gate`: nothing, or the optimiser's header (const evac::AdamHeader*) whose stop flag
// the kernels honour.  A unit instantiates the kernels of the forms it calls alone.
template <class... Gate>
inline void rpo_launch(const evac::RpoArgs& a, hipStream_t S, Gate... gate) {
    const size_t lds = evac::rpo_grad_lds_floats(a.D) * sizeof(float);
    const int tiles = (a.D + evac::kW1Tile - 1) / evac::kW1Tile;
    const dim3 fin((unsigned)(2 * evac::kFinishCombineWgs + 2 * tiles * a.S));
    if (a.norm_adv) hipLaunchKernelGGL(evac::k_rpo_adv_stats<Gate...>, dim3(1), dim3(evac::kFinishBlock), 0, S, a, gate...);
    hipLaunchKernelGGL(evac::k_rpo_grad<Gate...>, dim3((unsigned)a.P, 2u), dim3(evac::kGradBlock), lds, S, a, gate...);
    hipLaunchKernelGGL(evac::k_rpo_finish<Gate...>, fin, dim3(evac::kFinishBlock), 0, S, a, gate...);
}
}  // namespace
