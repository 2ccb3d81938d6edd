// Host side of the trainer's update for a population (include/evac.h: evac_rpo_update_population; kernels in evac_population.h):
// evac_rpo_update's checks and step loop, with the learner as one more grid dimension of each launch.  As in evac_train_api.hip:
// no handle, every refusal before the first HIP call, no device allocation, no synchronisation.
#include <hip/hip_runtime.h>

#include <cstddef>
#include <cstdint>
#include <mutex>

#include "evac_population.h"
#include "evac_population_host.h"

static_assert(evac::kMaxLearners == EVAC_MAX_LEARNERS, "evac::LearnerDraws holds EVAC_MAX_LEARNERS seeds and counters");
static_assert(sizeof(evac::RpoArgs) + sizeof(evac::LearnerStrides) + sizeof(evac::LearnerDraws) + sizeof(void*) <= 4096,
              "the gradient kernels' arguments must fit the kernel-argument segment");

namespace {
// wide observations: more dynamic LDS than the default limit; once per device (as rpo_raise_lds)
int raise_lds(int D, int dev) {
    if (evac::rpo_grad_lds_floats(D) * sizeof(float) <= 64 * 1024) return EVAC_OK;
    static std::mutex mu;
    static bool raised[64] = {};
    std::lock_guard<std::mutex> lock(mu);
    const int slot = dev >= 0 && dev < 64 ? dev : 0;
    if (!raised[slot]) {
        const size_t most = evac::rpo_grad_lds_floats(evac::kTrainMaxObs) * sizeof(float);
        if (hipFuncSetAttribute((const void*)evac::k_population_grad, hipFuncAttributeMaxDynamicSharedMemorySize, (int)most) != hipSuccess) {
            (void)hipGetLastError();
            return EVAC_ERR_HIP;
        }
        raised[slot] = true;
    }
    return EVAC_OK;
}
}  // namespace

namespace evac {
void population_launch_begin(AdamHeader* hdr, int64_t header_stride_bytes, int n_learners, hipStream_t stream) {
    hipLaunchKernelGGL(k_population_begin, dim3(1), dim3(kMaxLearners), 0, stream, hdr, header_stride_bytes, n_learners);
}
void population_launch_adv_stats(const RpoArgs& a, const LearnerStrides& q, const LearnerDraws& d, const AdamHeader* gate,
                                 int n_learners, hipStream_t stream) {
    hipLaunchKernelGGL(k_population_adv_stats, dim3(1, (unsigned)n_learners), dim3(kFinishBlock), 0, stream, a, q, d, gate);
}
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
    const int64_t B = learner_batch_size, M = n_minibatch, least = a.norm_adv ? 2 : 1;
    o.use_target_kl = use_target_kl != 0;
    o.target_kl = target_kl;
    const int dev = device_of(workspace);
    DeviceGuard g(dev);
    if (raise_lds(a.D, dev) != EVAC_OK) return EVAC_ERR_HIP;
    hipStream_t S = (hipStream_t)stream;
    const unsigned L = (unsigned)n_learners;
    evac::population_launch_begin(o.hdr, header_stride_bytes, n_learners, S);
    const size_t lds = evac::rpo_grad_lds_floats(a.D) * sizeof(float);
    const int tiles = (a.D + evac::kW1Tile - 1) / evac::kW1Tile;
    uint64_t k = 0;
    for (int32_t ep = 0; ep < n_epochs; ++ep) {
        for (int64_t start = 0; start < B; start += M) {
            const int64_t m = B - start < M ? B - start : M;
            if (m < least) continue;                   // (the tail: as evac_rpo_update skips it)
            const int64_t next = start + M, m_next = next >= B ? 0 : (B - next < M ? B - next : M);
            a.inds = perms + (int64_t)ep * B + start;
            a.noise = rpo_noise ? rpo_noise + k * (uint64_t)M * 2u : nullptr;
            a.stats = stats_out + k * 8u;
            rpo_shape(a, m, k);                        // (the kernels add the learner's first draw counter)
            o.sumsq = a.stats + 7;
            o.stats = a.stats;
            o.epoch_last = m_next < least;
            const evac::AdamHeader* gate = o.hdr;
            if (a.norm_adv) evac::population_launch_adv_stats(a, q, d, gate, n_learners, S);
            hipLaunchKernelGGL(evac::k_population_grad, dim3((unsigned)a.P, 2u, L), dim3(evac::kGradBlock), lds, S, a, q, d, gate);
            hipLaunchKernelGGL(evac::k_population_finish, dim3((unsigned)(2 * evac::kFinishCombineWgs + 2 * tiles * a.S), L),
                               dim3(evac::kFinishBlock), 0, S, a, q, d, gate);
            const int n = o.end[evac::kAdamTensors - 1];
            hipLaunchKernelGGL(evac::k_population_optimizer, dim3((unsigned)((n + evac::kAdamBlock - 1) / evac::kAdamBlock), L),
                               dim3(evac::kAdamBlock), 0, S, o, q);
            ++k;
        }
    }
    return hipGetLastError() == hipSuccess ? EVAC_OK : EVAC_ERR_HIP;
}

}  // extern "C"
