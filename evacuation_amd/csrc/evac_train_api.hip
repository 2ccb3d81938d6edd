// Host side of the trainer's update (include/evac.h: evac_gae .. evac_rpo_update; kernels in evac_train.h): argument checking
// and launches.  No handle and no env, so errors are reported through the return code alone and every refusal comes before the
// first HIP call.  No device allocation, no synchronisation: every call only enqueues work on the caller's stream.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstddef>
#include <cstdint>
#include <mutex>

#include "evac_host.h"
#include "evac_train.h"

extern "C" {

int evac_gae(int32_t n_steps, int64_t n_envs, const float* rewards, const float* values, const float* dones, const float* next_value,
             const float* next_done, double gamma, double gae_lambda, float* advantages_out, float* returns_out, void* stream) {
    if (n_steps < 1 || n_envs < 1 || n_envs >= (int64_t)1 << 38 || !rewards || !values || !dones || !next_value || !next_done ||
        !advantages_out || !returns_out)
        return EVAC_ERR_INVALID_ARGUMENT;
    DeviceGuard g(device_of(rewards));
    // gamma meets a tensor as float32; gamma * gae_lambda is a product of Python floats, rounded once (rpo_agent.py:217-219)
    hipLaunchKernelGGL(evac::k_gae, dim3((unsigned)((n_envs + 255) / 256)), dim3(256), 0, (hipStream_t)stream, (int)n_steps, n_envs,
                       rewards, values, dones, next_value, next_done, (float)gamma, (float)(gamma * gae_lambda), advantages_out,
                       returns_out);
    return hipGetLastError() == hipSuccess ? EVAC_OK : EVAC_ERR_HIP;
}

int64_t evac_rpo_workspace_bytes(int32_t obs_dim, int64_t n_minibatch) {
    if (obs_dim < 1 || obs_dim > evac::kTrainMaxObs || n_minibatch < 1 || n_minibatch >= (int64_t)1 << 31) return EVAC_ERR_INVALID_ARGUMENT;
    return (int64_t)evac::kWsFixedBytes + 2 * n_minibatch * evac::kTrainHidden * (int64_t)sizeof(float) +
           (int64_t)evac::rpo_w1_parts_floats(obs_dim, n_minibatch) * (int64_t)sizeof(float) +
           2 * (int64_t)evac::rpo_parts_upper(n_minibatch) * evac::kPart * (int64_t)sizeof(float);
}

namespace {
// What evac_rpo_minibatch_grad checks and sets up, for every entry that runs the gradient of a minibatch.
int rpo_prepare(const evac_mlp_policy_t* policy, const evac_rpo_loss_config_t* cfg, int64_t batch_size, const float* b_obs,
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
void rpo_shape(evac::RpoArgs& a, int64_t n_minibatch, uint64_t draw_counter) {
    a.M = (int)n_minibatch;
    const int p0 = evac::rpo_parts_upper(n_minibatch);
    a.chunk = (int)((n_minibatch + p0 - 1) / p0);
    a.P = (int)((n_minibatch + a.chunk - 1) / a.chunk);            // every workgroup has samples (P <= p0: the workspace's bound)
    a.S = evac::rpo_w1_segments(a.D, n_minibatch);
    a.ctr_lo = (uint32_t)draw_counter; a.ctr_hi = (uint32_t)(draw_counter >> 32);
}
// wide observations: more dynamic LDS than the default limit; once per device and kernel
int rpo_raise_lds(const evac::RpoArgs& a, int dev, bool gated) {
    if (evac::rpo_grad_lds_floats(a.D) * sizeof(float) <= 64 * 1024) return EVAC_OK;
    static std::mutex mu;
    static bool raised[2][64] = {};
    std::lock_guard<std::mutex> lock(mu);
    const int slot = dev >= 0 && dev < 64 ? dev : 0;
    if (!raised[gated][slot]) {
        const size_t most = evac::rpo_grad_lds_floats(evac::kTrainMaxObs) * sizeof(float);
        const void* fn = gated ? (const void*)evac::k_rpo_grad<const evac::AdamHeader*> : (const void*)evac::k_rpo_grad<>;
        if (hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)most) != hipSuccess) {
            (void)hipGetLastError();
            return EVAC_ERR_HIP;
        }
        raised[gated][slot] = true;
    }
    return EVAC_OK;
}
// the launches of one minibatch's gradient; `gate` = the optimiser's header whose stop flag the kernels honour, or NULL
void rpo_launch(const evac::RpoArgs& a, hipStream_t S, const evac::AdamHeader* gate) {
    const size_t lds = evac::rpo_grad_lds_floats(a.D) * sizeof(float);
    const int tiles = (a.D + evac::kW1Tile - 1) / evac::kW1Tile;
    const dim3 fin((unsigned)(2 * evac::kFinishCombineWgs + 2 * tiles * a.S));
    if (!gate) {
        if (a.norm_adv) hipLaunchKernelGGL(evac::k_rpo_adv_stats<>, dim3(1), dim3(evac::kFinishBlock), 0, S, a);
        hipLaunchKernelGGL(evac::k_rpo_grad<>, dim3((unsigned)a.P, 2u), dim3(evac::kGradBlock), lds, S, a);
        hipLaunchKernelGGL(evac::k_rpo_finish<>, fin, dim3(evac::kFinishBlock), 0, S, a);
    } else {
        if (a.norm_adv) hipLaunchKernelGGL(evac::k_rpo_adv_stats<const evac::AdamHeader*>, dim3(1), dim3(evac::kFinishBlock), 0, S, a, gate);
        hipLaunchKernelGGL(evac::k_rpo_grad<const evac::AdamHeader*>, dim3((unsigned)a.P, 2u), dim3(evac::kGradBlock), lds, S, a, gate);
        hipLaunchKernelGGL(evac::k_rpo_finish<const evac::AdamHeader*>, fin, dim3(evac::kFinishBlock), 0, S, a, gate);
    }
}

// What evac_adam_step checks and sets up.  (!(x > 0) also refuses a NaN.)
int adam_prepare(const evac_mlp_policy_grads_t* params, const evac_mlp_policy_grads_t* grads, const evac_adam_state_t* state,
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
    const int H = evac::kTrainHidden, D = obs_dim;
    const int n[evac::kAdamTensors] = {H * D, H, H * H, H, 2 * H, 2, 2, H * D, H, H * H, H, H, 1};
    int end = 0;
    for (int i = 0; i < evac::kAdamTensors; ++i) a.end[i] = (end += n[i]);
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
void adam_launch(const evac::AdamArgs& a, hipStream_t S) {
    const int n = a.end[evac::kAdamTensors - 1];
    hipLaunchKernelGGL(evac::k_adam, dim3((unsigned)((n + evac::kAdamBlock - 1) / evac::kAdamBlock)), dim3(evac::kAdamBlock), 0, S, a);
}
// evac_rpo_minibatch_grad, and with `adam` the optimiser's launch after it (evac_rpo_minibatch_step)
int rpo_minibatch(const evac_mlp_policy_t* policy, const evac_rpo_loss_config_t* cfg, int64_t batch_size, const float* b_obs,
                  const float* b_actions, const float* b_logprobs, const float* b_advantages, const float* b_returns,
                  const float* b_values, int64_t n_minibatch, const int64_t* mb_inds, const float* rpo_noise, uint64_t seed,
                  uint64_t draw_counter, const evac_mlp_policy_grads_t* grads_out, float* stats_out, void* workspace, void* stream,
                  bool adam, const evac_mlp_policy_grads_t* params, const evac_adam_state_t* state, const evac_adam_config_t* adam_cfg) {
    evac::RpoArgs a;
    int rc = rpo_prepare(policy, cfg, batch_size, b_obs, b_actions, b_logprobs, b_advantages, b_returns, b_values, n_minibatch,
                         mb_inds, rpo_noise, seed, grads_out, stats_out, workspace, a);
    if (rc != EVAC_OK) return rc;
    evac::AdamArgs o;
    if (adam) {
        rc = adam_prepare(params, grads_out, state, adam_cfg, policy->obs_dim, o);
        if (rc != EVAC_OK) return rc;
        o.sumsq = stats_out + 7;
    }
    rpo_shape(a, n_minibatch, draw_counter);
    const int dev = device_of(workspace);
    DeviceGuard g(dev);
    if (rpo_raise_lds(a, dev, false) != EVAC_OK) return EVAC_ERR_HIP;
    rpo_launch(a, (hipStream_t)stream, nullptr);
    if (adam) adam_launch(o, (hipStream_t)stream);
    return hipGetLastError() == hipSuccess ? EVAC_OK : EVAC_ERR_HIP;
}
}  // namespace

int evac_rpo_minibatch_grad(const evac_mlp_policy_t* policy, const evac_rpo_loss_config_t* cfg, int64_t batch_size, const float* b_obs,
                            const float* b_actions, const float* b_logprobs, const float* b_advantages, const float* b_returns,
                            const float* b_values, int64_t n_minibatch, const int64_t* mb_inds, const float* rpo_noise,
                            uint64_t seed, uint64_t draw_counter, const evac_mlp_policy_grads_t* grads_out, float* stats_out,
                            void* workspace, void* stream) {
    return rpo_minibatch(policy, cfg, batch_size, b_obs, b_actions, b_logprobs, b_advantages, b_returns, b_values, n_minibatch, mb_inds,
                         rpo_noise, seed, draw_counter, grads_out, stats_out, workspace, stream, false, nullptr, nullptr, nullptr);
}

int evac_adam_step(const evac_mlp_policy_grads_t* params, const evac_mlp_policy_grads_t* grads, const evac_adam_state_t* state,
                   const evac_adam_config_t* cfg, int32_t obs_dim, const float* grad_sumsq, void* stream) {
    evac::AdamArgs a;
    const int rc = adam_prepare(params, grads, state, cfg, obs_dim, a);
    if (rc != EVAC_OK) return rc;
    if (!grad_sumsq) return EVAC_ERR_INVALID_ARGUMENT;
    a.sumsq = grad_sumsq;
    DeviceGuard g(device_of(state->header));
    adam_launch(a, (hipStream_t)stream);
    return hipGetLastError() == hipSuccess ? EVAC_OK : EVAC_ERR_HIP;
}

int evac_rpo_minibatch_step(const evac_mlp_policy_t* policy, const evac_rpo_loss_config_t* cfg, int64_t batch_size, const float* b_obs,
                            const float* b_actions, const float* b_logprobs, const float* b_advantages, const float* b_returns,
                            const float* b_values, int64_t n_minibatch, const int64_t* mb_inds, const float* rpo_noise,
                            uint64_t seed, uint64_t draw_counter, const evac_mlp_policy_grads_t* grads_out, float* stats_out,
                            void* workspace, void* stream, const evac_mlp_policy_grads_t* params, const evac_adam_state_t* state,
                            const evac_adam_config_t* adam_cfg) {
    return rpo_minibatch(policy, cfg, batch_size, b_obs, b_actions, b_logprobs, b_advantages, b_returns, b_values, n_minibatch, mb_inds,
                         rpo_noise, seed, draw_counter, grads_out, stats_out, workspace, stream, true, params, state, adam_cfg);
}

int evac_rpo_update(const evac_mlp_policy_t* policy, const evac_mlp_policy_grads_t* params, const evac_mlp_policy_grads_t* grads,
                    const evac_rpo_loss_config_t* loss_cfg, const evac_adam_config_t* adam_cfg, const evac_adam_state_t* state,
                    int64_t batch_size, const float* b_obs, const float* b_actions, const float* b_logprobs, const float* b_advantages,
                    const float* b_returns, const float* b_values, int64_t n_minibatch, int32_t n_epochs, const int64_t* perms,
                    const float* rpo_noise, uint64_t seed, uint64_t first_draw_counter, int32_t use_target_kl, double target_kl,
                    float* stats_out, void* workspace, void* stream) {
    if (n_epochs < 1) return EVAC_ERR_INVALID_ARGUMENT;
    evac::RpoArgs a;
    int rc = rpo_prepare(policy, loss_cfg, batch_size, b_obs, b_actions, b_logprobs, b_advantages, b_returns, b_values, n_minibatch,
                         perms, rpo_noise, seed, grads, stats_out, workspace, a);
    if (rc != EVAC_OK) return rc;
    evac::AdamArgs o;
    rc = adam_prepare(params, grads, state, adam_cfg, policy->obs_dim, o);
    if (rc != EVAC_OK) return rc;
    o.gated = 1;
    o.use_target_kl = use_target_kl != 0;
    o.target_kl = target_kl;
    const int dev = device_of(workspace);
    DeviceGuard g(dev);
    if (rpo_raise_lds(a, dev, true) != EVAC_OK) return EVAC_ERR_HIP;
    hipStream_t S = (hipStream_t)stream;
    // stop, steps_run, epochs_run (and the ticket, zero anyway)
    if (hipMemsetAsync((char*)state->header + offsetof(evac::AdamHeader, stop), 0, 16, S) != hipSuccess) {
        (void)hipGetLastError();
        return EVAC_ERR_HIP;
    }
    const int64_t B = batch_size, M = n_minibatch, least = a.norm_adv ? 2 : 1;
    uint64_t k = 0;
    for (int32_t ep = 0; ep < n_epochs; ++ep) {
        for (int64_t start = 0; start < B; start += M) {
            const int64_t m = B - start < M ? B - start : M;
            if (m < least) continue;                   // (the tail: as RPOTrainer.update() skips it)
            const int64_t next = start + M, m_next = next >= B ? 0 : (B - next < M ? B - next : M);
            a.inds = perms + (int64_t)ep * B + start;
            a.noise = rpo_noise ? rpo_noise + k * (uint64_t)M * 2u : nullptr;
            a.stats = stats_out + k * 8u;
            rpo_shape(a, m, first_draw_counter + k);
            o.sumsq = a.stats + 7;
            o.stats = a.stats;
            o.epoch_last = m_next < least;
            rpo_launch(a, S, o.hdr);
            adam_launch(o, S);
            ++k;
        }
    }
    return hipGetLastError() == hipSuccess ? EVAC_OK : EVAC_ERR_HIP;
}

}  // extern "C"
