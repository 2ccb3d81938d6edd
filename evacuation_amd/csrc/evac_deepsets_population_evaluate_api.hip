// Host side of the evaluation of a population of deep-sets leaders (include/evac.h: evac_policy_evaluate_population_deepsets;
// kernel in evac_deepsets_population_evaluate.h).  The entry is evac_handle_host.h's encoder_evaluate with the learners' shares
// (evac_deepsets_host.h's DeepSetsLearnerShares, which the collection entry of evac_deepsets_population_api.hip shares): every
// refusal before the first HIP call, the handle joined, one kernel on the stream, no synchronisation.  A unit of its own: the
// kernel lists of evac_deepsets_api.hip and evac_deepsets_population_api.hip stay what they are.
#include <hip/hip_runtime.h>

#include <cstddef>
#include <cstdint>
#include <string>

#define EVAC_TEMPLATE_KERNELS_ONLY      // (evac_device.h: its plain kernels live in evac_api.hip)
#include "evac_deepsets_population_evaluate.h"
#include "evac_deepsets_host.h"
#include "evac_handle_host.h"
#include "evac_host.h"

static_assert(sizeof(evac::Params) + sizeof(evac::PolicyArgs) + sizeof(evac::EvalArgs) + sizeof(evac::PopulationArgs) +
                      sizeof(evac::DeepSetsArgs) + sizeof(evac::DeepSetsStrides) + 8 <= 4096,
              "k_evaluate_population_deepsets: arguments beyond the kernel-argument segment");
static_assert(sizeof(evac::PolicyFamily::Smem) + sizeof(evac::PolicySmem<false>) + sizeof(evac::EvalSmem) + sizeof(evac::DeepSetsSmem) <=
                  160 * 1024, "k_evaluate_population_deepsets: LDS beyond a CU's 160 KiB");

namespace {

// evac_handle_host.h's trait of an encoder, for the population's evaluation entry (the lone kernels are evac_deepsets_api.hip's)
struct DeepSetsPopulationEncoder : DeepSetsEncoderHost {
    static constexpr const char* kEvaluatePopulation = "evac_policy_evaluate_population_deepsets";
};
// ... and its learners: the shares and strides of evac_deepsets_host.h, whose ids the learners' envs draw with, the launch
struct DeepSetsEvaluateLearners : DeepSetsLearnerShares {
    int shared;

    void launch(const evac_host::HandleView& v, const evac::PolicyArgs& a, const evac::EvalArgs& ev, const evac::DeepSetsArgs& ea,
                hipStream_t S) const {
        const auto fn = EVAC_PICK_BOOL2(evac::k_evaluate_population_deepsets, ev.norm_state != nullptr, v.default_cfg);
        hipLaunchKernelGGL(fn, dim3((unsigned)(n_learners * q.wgs)), dim3(evac::PolicyFamily::kBlock), 0, S, v.p, a, ev, q, ea, dq, shared);
    }
};

}  // namespace

extern "C" {

int evac_policy_evaluate_population_deepsets(evac_handle_t h, int32_t n_learners, const evac_mlp_policy_t* policy,
                                             const evac_mlp_policy_strides_t* strides, const evac_deepsets_t* encoder,
                                             const evac_deepsets_strides_t* enc_strides, int32_t agent, int32_t shared_episodes,
                                             int32_t n_episodes, int32_t max_steps, int32_t* progress, evac_episode_stats_t* episodes_out,
                                             const double* norm_state, float obs_clip, float epsilon, void* stream) {
    return encoder_evaluate<DeepSetsPopulationEncoder, false, DeepSetsEvaluateLearners>(
        h, agent, policy, n_episodes, max_steps, progress, episodes_out, norm_state, obs_clip, epsilon, encoder, stream, nullptr,
        DeepSetsEvaluateLearners{{n_learners, strides, enc_strides}, (int)(shared_episodes != 0)});
}

}  // extern "C"
