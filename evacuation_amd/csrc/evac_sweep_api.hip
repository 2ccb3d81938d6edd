// Host side of a population with a configuration per learner (include/evac.h: evac_gae_learners, evac_rpo_update_sweep; kernels
// in evac_sweep.h): evac_rpo_update_population's checks and step loop (evac_train_host.h) with the learners' values beside their
// seeds in the kernel arguments.  As in evac_population_api.hip: no handle, every refusal before the first HIP call, no device
// allocation, no synchronisation.  The launches that read no hyperparameter (the begin and the advantage statistics) are
// evac_population_api.hip's own, reached through evac_population_host.h.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstddef>
#include <cstdint>

#include "evac_population_host.h"
#include "evac_sweep.h"
#include "evac_sweep_host.h"

static_assert(sizeof(evac_learner_hyper_t) == 56, "evac_learner_hyper_t: four doubles, five floats, one int32");
// every kernel's arguments against the 4 KiB of the kernel-argument segment
static_assert(sizeof(evac::RpoArgs) + sizeof(evac::LearnerStrides) + sizeof(evac::LearnerDraws) + sizeof(evac::LearnerLoss) +
                      sizeof(void*) <= 4096, "k_sweep_grad / k_sweep_finish: arguments beyond the kernel-argument segment");
static_assert(sizeof(evac::AdamArgs) + sizeof(evac::LearnerStrides) + sizeof(evac::LearnerSteps) <= 4096,
              "k_sweep_optimizer: arguments beyond the kernel-argument segment");
static_assert(4 + 8 + 5 * sizeof(void*) + 8 + sizeof(evac::LearnerDiscounts) + 2 * sizeof(void*) + 8 <= 4096,
              "k_sweep_advantages: arguments beyond the kernel-argument segment");

// The launches the sweeps of the encoder leaders reuse on their common encoded batch (evac_sweep_host.h)
namespace evac {
void sweep_launch_grad(const RpoArgs& a, const LearnerStrides& q, const LearnerDraws& d, const LearnerLoss& h, const AdamHeader* gate,
                       dim3 grid, size_t lds, hipStream_t stream) {
    hipLaunchKernelGGL(k_sweep_grad, grid, dim3(kGradBlock), lds, stream, a, q, d, h, gate);
}
void sweep_launch_finish(const RpoArgs& a, const LearnerStrides& q, const LearnerDraws& d, const LearnerLoss& h, const AdamHeader* gate,
                         dim3 grid, hipStream_t stream) {
    hipLaunchKernelGGL(k_sweep_finish, grid, dim3(kFinishBlock), 0, stream, a, q, d, h, gate);
}
int sweep_raise_grad_lds(int D, int dev) { return rpo_raise_lds<k_sweep_grad>(D, dev); }
}  // namespace evac

extern "C" {

int evac_gae_learners(int32_t n_steps, int64_t n_envs, const float* rewards, const float* values, const float* dones,
                      const float* next_value, const float* next_done, int64_t envs_per_learner, int32_t n_learners,
                      const evac_learner_hyper_t* hypers, float* advantages_out, float* returns_out, void* stream) {
    if (n_steps < 1 || n_envs < 1 || n_envs >= (int64_t)1 << 38 || !rewards || !values || !dones || !next_value || !next_done ||
        !advantages_out || !returns_out)
        return EVAC_ERR_INVALID_ARGUMENT;
    if (!learner_hypers_ok(hypers, n_learners) || envs_per_learner < 1 || n_envs / n_learners != envs_per_learner ||
        n_envs % n_learners != 0)
        return EVAC_ERR_INVALID_ARGUMENT;
    evac::LearnerDiscounts h{};
    for (int s = 0; s < n_learners; ++s) {
        // as evac_gae: gamma meets a tensor as float32; gamma * gae_lambda is a product of Python floats, rounded once
        h.gamma[s] = (float)hypers[s].gamma;
        h.gl[s] = (float)(hypers[s].gamma * hypers[s].gae_lambda);
    }
    DeviceGuard g(device_of(rewards));
    hipLaunchKernelGGL(evac::k_sweep_advantages, dim3((unsigned)((n_envs + 255) / 256)), dim3(256), 0, (hipStream_t)stream, (int)n_steps,
                       n_envs, rewards, values, dones, next_value, next_done, envs_per_learner, h, advantages_out, returns_out);
    return hipGetLastError() == hipSuccess ? EVAC_OK : EVAC_ERR_HIP;
}

int evac_rpo_update_sweep(int32_t n_learners, const evac_mlp_policy_t* policy, const evac_mlp_policy_grads_t* params,
                          const evac_mlp_policy_grads_t* grads, const evac_mlp_policy_strides_t* param_strides,
                          const evac_mlp_policy_strides_t* grad_strides, const evac_mlp_policy_strides_t* moment_strides,
                          int64_t header_stride_bytes, const evac_rpo_loss_config_t* loss_cfg, const evac_adam_config_t* adam_cfg,
                          const evac_adam_state_t* state, int64_t batch_size, const float* b_obs, const float* b_actions,
                          const float* b_logprobs, const float* b_advantages, const float* b_returns, const float* b_values,
                          int64_t learner_batch_size, int64_t n_minibatch, int32_t n_epochs, const int64_t* perms,
                          const float* rpo_noise, const uint64_t* seeds, const uint64_t* first_draw_counters,
                          const evac_learner_hyper_t* hypers, float* stats_out, void* workspace, void* stream) {
    evac::RpoArgs a;
    evac::AdamArgs o;
    evac::LearnerStrides q;
    evac::LearnerDraws d;
    const int rc = population_prepare(n_learners, policy, params, grads, param_strides, grad_strides, moment_strides, header_stride_bytes,
                                      loss_cfg, adam_cfg, state, batch_size, b_obs, b_actions, b_logprobs, b_advantages, b_returns,
                                      b_values, learner_batch_size, n_minibatch, n_epochs, perms, rpo_noise, seeds, first_draw_counters,
                                      stats_out, workspace, a, o, q, d);
    if (rc != EVAC_OK) return rc;
    if (!learner_hypers_ok(hypers, n_learners)) return EVAC_ERR_INVALID_ARGUMENT;
    evac::LearnerLoss hl;
    evac::LearnerSteps hs;
    learner_values(hypers, n_learners, hl, hs);
    const int dev = device_of(workspace);
    DeviceGuard g(dev);
    if (rpo_raise_lds<evac::k_sweep_grad>(a.D, dev) != EVAC_OK) return EVAC_ERR_HIP;
    hipStream_t S = (hipStream_t)stream;
    evac::population_launch_begin(o.hdr, header_stride_bytes, n_learners, S);
    // (draw counter base 0: the kernels add the learner's first draw counter)
    rpo_update_steps(a, o, learner_batch_size, n_minibatch, n_epochs, perms, rpo_noise, stats_out, 0,
                     [&](const evac::RpoArgs& step, const evac::AdamArgs& adam, uint64_t) {
                         const LearnerGrids grid = learner_grids(step, adam, (unsigned)n_learners);
                         const evac::AdamHeader* gate = adam.hdr;
                         if (step.norm_adv) evac::population_launch_adv_stats(step, q, d, gate, n_learners, S);
                         hipLaunchKernelGGL(evac::k_sweep_grad, grid.grad, dim3(evac::kGradBlock), grid.lds, S, step, q, d, hl, gate);
                         hipLaunchKernelGGL(evac::k_sweep_finish, grid.finish, dim3(evac::kFinishBlock), 0, S, step, q, d, hl, gate);
                         hipLaunchKernelGGL(evac::k_sweep_optimizer, grid.optimizer, dim3(evac::kAdamBlock), 0, S, adam, q, hs);
                     });
    return hipGetLastError() == hipSuccess ? EVAC_OK : EVAC_ERR_HIP;
}

}  // extern "C"
