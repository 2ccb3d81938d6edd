// Host side of the trainer's update for a population (include/evac.h: evac_rpo_update_population; kernels in evac_population.h):
// evac_rpo_update's checks and step loop (evac_train_host.h), with the learner as one more grid dimension of each launch.  As in
// evac_train_api.hip: no handle, every refusal before the first HIP call, no device allocation, no synchronisation.
#include <hip/hip_runtime.h>

#include <cstddef>
#include <cstdint>

#include "evac_population.h"
#include "evac_population_host.h"

static_assert(sizeof(evac::RpoArgs) + sizeof(evac::LearnerStrides) + sizeof(evac::LearnerDraws) + sizeof(void*) <= 4096,
              "the gradient kernels' arguments must fit the kernel-argument segment");

namespace evac {
void population_launch_begin(AdamHeader* hdr, int64_t header_stride_bytes, int n_learners, hipStream_t stream) {
    hipLaunchKernelGGL(k_population_begin, dim3(1), dim3(kMaxLearners), 0, stream, hdr, header_stride_bytes, n_learners);
}
void population_launch_adv_stats(const RpoArgs& a, const LearnerStrides& q, const LearnerDraws& d, const AdamHeader* gate,
                                 int n_learners, hipStream_t stream) {
    hipLaunchKernelGGL(k_population_adv_stats, dim3(1, (unsigned)n_learners), dim3(kFinishBlock), 0, stream, a, q, d, gate);
}
void population_launch_grad(const RpoArgs& a, const LearnerStrides& q, const LearnerDraws& d, const AdamHeader* gate, dim3 grid,
                            size_t lds, hipStream_t stream) {
    hipLaunchKernelGGL(k_population_grad, grid, dim3(kGradBlock), lds, stream, a, q, d, gate);
}
void population_launch_finish(const RpoArgs& a, const LearnerStrides& q, const LearnerDraws& d, const AdamHeader* gate, dim3 grid,
                              hipStream_t stream) {
    hipLaunchKernelGGL(k_population_finish, grid, dim3(kFinishBlock), 0, stream, a, q, d, gate);
}
int population_raise_grad_lds(int D, int dev) { return rpo_raise_lds<k_population_grad>(D, dev); }
}  // namespace evac

extern "C" {

int64_t evac_rpo_population_workspace_bytes(int32_t obs_dim, int64_t n_minibatch, int32_t n_learners) {
    if (n_learners < 1 || n_learners > EVAC_MAX_LEARNERS) return EVAC_ERR_INVALID_ARGUMENT;
    const int64_t one = slice_bytes(obs_dim, n_minibatch);
    return one < 0 ? one : one * n_learners;
}

int evac_rpo_update_population(int32_t n_learners, const evac_mlp_policy_t* policy, const evac_mlp_policy_grads_t* params,
                               const evac_mlp_policy_grads_t* grads, const evac_mlp_policy_strides_t* param_strides,
                               const evac_mlp_policy_strides_t* grad_strides, const evac_mlp_policy_strides_t* moment_strides,
                               int64_t header_stride_bytes, const evac_rpo_loss_config_t* loss_cfg, const evac_adam_config_t* adam_cfg,
                               const evac_adam_state_t* state, int64_t batch_size, const float* b_obs, const float* b_actions,
                               const float* b_logprobs, const float* b_advantages, const float* b_returns, const float* b_values,
                               int64_t learner_batch_size, int64_t n_minibatch, int32_t n_epochs, const int64_t* perms,
                               const float* rpo_noise, const uint64_t* seeds, const uint64_t* first_draw_counters,
                               int32_t use_target_kl, double target_kl, float* stats_out, void* workspace, void* stream) {
    evac::RpoArgs a;
    evac::AdamArgs o;
    evac::LearnerStrides q;
    evac::LearnerDraws d;
    const int rc = population_prepare(n_learners, policy, params, grads, param_strides, grad_strides, moment_strides, header_stride_bytes,
                                      loss_cfg, adam_cfg, state, batch_size, b_obs, b_actions, b_logprobs, b_advantages, b_returns,
                                      b_values, learner_batch_size, n_minibatch, n_epochs, perms, rpo_noise, seeds, first_draw_counters,
                                      stats_out, workspace, a, o, q, d);
    if (rc != EVAC_OK) return rc;
    o.use_target_kl = use_target_kl != 0;
    o.target_kl = target_kl;
    const int dev = device_of(workspace);
    DeviceGuard g(dev);
    if (evac::population_raise_grad_lds(a.D, dev) != EVAC_OK) return EVAC_ERR_HIP;
    hipStream_t S = (hipStream_t)stream;
    evac::population_launch_begin(o.hdr, header_stride_bytes, n_learners, S);
    // (draw counter base 0: the kernels add the learner's first draw counter)
    rpo_update_steps(a, o, learner_batch_size, n_minibatch, n_epochs, perms, rpo_noise, stats_out, 0,
                     [&](const evac::RpoArgs& step, const evac::AdamArgs& adam, uint64_t) {
                         const LearnerGrids grid = learner_grids(step, adam, (unsigned)n_learners);
                         const evac::AdamHeader* gate = adam.hdr;
                         if (step.norm_adv) evac::population_launch_adv_stats(step, q, d, gate, n_learners, S);
                         evac::population_launch_grad(step, q, d, gate, grid.grad, grid.lds, S);
                         evac::population_launch_finish(step, q, d, gate, grid.finish, S);
                         hipLaunchKernelGGL(evac::k_population_optimizer, grid.optimizer, dim3(evac::kAdamBlock), 0, S, adam, q);
                     });
    return hipGetLastError() == hipSuccess ? EVAC_OK : EVAC_ERR_HIP;
}

}  // extern "C"
