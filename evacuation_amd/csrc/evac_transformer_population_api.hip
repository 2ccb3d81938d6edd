// Host side of the collection of a population of transformer leaders (include/evac.h: evac_policy_rollout_population_transformer;
// kernel in evac_transformer_population.h).  The entry is evac_handle_host.h's encoder_rollout with the learners' shares
// (evac_transformer_env_host.h's TransformerLearnerShares, which the evaluation entry of
// evac_transformer_population_evaluate_api.hip shares): every refusal before the first HIP call, the handle joined, one kernel on the
// stream, no synchronisation.  A unit of its own: the kernel list of evac_transformer_api.hip stays what it is.  The update of
// such a population is evac_transformer_population_update_api.hip's, its sweep evac_transformer_sweep_api.hip's.
#include <hip/hip_runtime.h>

#include <cstddef>
#include <cstdint>
#include <string>

#define EVAC_TEMPLATE_KERNELS_ONLY      // (evac_device.h: its plain kernels live in evac_api.hip)
#include "evac_transformer_population.h"
#include "evac_handle_host.h"
#include "evac_host.h"
#include "evac_transformer_env_host.h"

static_assert(sizeof(evac::Params) + 8 + sizeof(evac::PolicyArgs) + sizeof(evac::NormArgs) + sizeof(evac::PopulationArgs) +
                      sizeof(evac::TransformerArgs) + sizeof(evac::TransformerStrides) <= 4096,
              "k_collect_population_transformer: arguments beyond the kernel-argument segment");
static_assert(sizeof(evac::PolicyFamily::Smem) + sizeof(evac::PolicySmem<false>) + sizeof(evac::TransformerSmem) <= 160 * 1024,
              "k_collect_population_transformer: LDS beyond a CU's 160 KiB");

namespace evac {
void transformer_population_launch_collect(const evac_host::HandleView& v, int n_steps, const PolicyArgs& a, const NormArgs& na,
                                           int n_learners, const PopulationArgs& q, const TransformerArgs& ea,
                                           const TransformerStrides& tq, hipStream_t stream) {
    const auto fn = EVAC_PICK_BOOL2(k_collect_population_transformer, na.state != nullptr, v.default_cfg);
    hipLaunchKernelGGL(fn, dim3((unsigned)(n_learners * q.wgs)), dim3(PolicyFamily::kBlock), 0, stream, v.p, n_steps, a, na, q, ea, tq);
}
}  // namespace evac

namespace {

// evac_handle_host.h's trait of an encoder, for the population's collection entry (the lone kernels are evac_transformer_api.hip's)
struct TransformerPopulationEncoder : TransformerEncoderHost {
    static constexpr const char* kRollout = "evac_policy_rollout_population_transformer";
};
// ... and its learners: their shares of the handle's envs and the strides of their tensors (evac_transformer_env_host.h), the launch
struct TransformerLearners : TransformerLearnerShares {
    void launch(const evac_host::HandleView& v, int n_steps, const evac::PolicyArgs& a, const evac::NormArgs& na,
                const evac::TransformerArgs& ea, hipStream_t S) const {
        evac::transformer_population_launch_collect(v, n_steps, a, na, n_learners, q, ea, tq, S);
    }
};

}  // namespace

extern "C" {

int evac_policy_rollout_population_transformer(evac_handle_t h, int32_t n_learners, const evac_mlp_policy_t* policy,
                                               const evac_mlp_policy_strides_t* strides, const evac_transformer_t* encoder,
                                               const evac_transformer_strides_t* enc_strides, int32_t n_steps, float* next_obs,
                                               float* next_done, float* obs_out, float* actions_out, float* logprob_out,
                                               float* value_out, float* reward_out, float* done_out, float* next_value_out,
                                               evac_episode_stats_t* final_stats, double* norm_state, float gamma, float obs_clip,
                                               float reward_clip, float epsilon, void* stream) {
    return encoder_rollout<TransformerPopulationEncoder>(h, n_steps, policy,
                                                         collect_outputs(next_obs, next_done, obs_out, actions_out, logprob_out, value_out,
                                                                         reward_out, done_out, next_value_out, final_stats),
                                                         evac::NormArgs{norm_state, gamma, obs_clip, reward_clip, epsilon}, encoder, stream,
                                                         TransformerLearners{{n_learners, strides, enc_strides}});
}

}  // extern "C"
