// Host side of the trainer's update (include/evac.h: evac_gae .. evac_rpo_update; kernels in evac_train.h): argument checking
// and launches.  No handle and no env, so errors are reported through the return code alone and every refusal comes before the
// first HIP call.  No device allocation, no synchronisation: every call only enqueues work on the caller's stream.
#include <hip/hip_runtime.h>

#include <cstddef>
#include <cstdint>

#include "evac_train_host.h"

// The two kernels of evac_train.h that are not templates: defined in this translation unit alone.
namespace evac {

// ---- rpo_agent.py:205-220: advantages[t] = delta_t + gamma lambda nonterminal_{t+1} advantages[t+1], one lane per env ----
// The reference's torch ops, operation for operation (every product and sum rounded: no fma), so the result is bit-equal to the
// float32 loop on the CPU.  `gl` = (float)(gamma * gae_lambda), the product formed in double and rounded once (Python floats).
// TWIN: k_sweep_advantages (evac_sweep.h) repeats the loop; change one, change the other.
__global__ __launch_bounds__(256) void k_gae(int T, int64_t E, const float* __restrict__ rewards, const float* __restrict__ values,
                                             const float* __restrict__ dones, const float* __restrict__ next_value,
                                             const float* __restrict__ next_done, float gamma, float gl, float* __restrict__ adv_out,
                                             float* __restrict__ ret_out) {
    const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (e >= E) return;
    float vn = next_value[e], dn = next_done[e], last = 0.0f;
    for (int t = T - 1; t >= 0; --t) {
        const size_t i = (size_t)t * (size_t)E + (size_t)e;
        const float r = rewards[i], v = values[i], d = dones[i];
        const float nonterminal = __fsub_rn(1.0f, dn);
        const float delta = __fsub_rn(__fadd_rn(r, __fmul_rn(__fmul_rn(gamma, vn), nonterminal)), v);
        last = __fadd_rn(delta, __fmul_rn(__fmul_rn(gl, nonterminal), last));
        adv_out[i] = last;
        ret_out[i] = __fadd_rn(last, v);
        vn = v;
        dn = d;
    }
}

__global__ __launch_bounds__(kAdamBlock) void k_adam(AdamArgs a) {
    if (a.gated && a.hdr->stop) return;
    adam_stage(a);
}

}  // namespace evac

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
    if (rpo_raise_lds<evac::k_rpo_grad<>>(a.D, dev) != EVAC_OK) return EVAC_ERR_HIP;
    rpo_launch(a, (hipStream_t)stream);
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
    if (rpo_raise_lds<evac::k_rpo_grad<const evac::AdamHeader*>>(a.D, dev) != EVAC_OK) return EVAC_ERR_HIP;
    hipStream_t S = (hipStream_t)stream;
    // stop, steps_run, epochs_run (and the ticket, zero anyway)
    if (hipMemsetAsync((char*)state->header + offsetof(evac::AdamHeader, stop), 0, 16, S) != hipSuccess) {
        (void)hipGetLastError();
        return EVAC_ERR_HIP;
    }
    rpo_update_steps(a, o, batch_size, n_minibatch, n_epochs, perms, rpo_noise, stats_out, first_draw_counter,
                     [S](const evac::RpoArgs& step, const evac::AdamArgs& adam, uint64_t) {
                         rpo_launch(step, S, (const evac::AdamHeader*)adam.hdr);
                         adam_launch(adam, S);
                     });
    return hipGetLastError() == hipSuccess ? EVAC_OK : EVAC_ERR_HIP;
}

}  // extern "C"
