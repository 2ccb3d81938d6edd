// Host side of the transformer leader (include/evac.h: evac_policy_rollout_transformer, evac_policy_evaluate_transformer; kernels
// in evac_transformer.h): the encoder's blocks beside the actor-critic's thirteen tensors.  The two entries' bodies -- the checks
// in their order, the handle, the launch -- are evac_handle_host.h's encoder_rollout / encoder_evaluate, which
// evac_deepsets_api.hip shares; this unit holds what is the attention encoder's own: its limits, its check, its kernels.
#include <hip/hip_runtime.h>

#include <cstddef>
#include <cstdint>
#include <string>

#define EVAC_TEMPLATE_KERNELS_ONLY      // (evac_device.h: its plain kernels live in evac_api.hip)
#include "evac_transformer.h"
#include "evac_handle_host.h"
#include "evac_host.h"
#include "evac_transformer_host.h"

static_assert(sizeof(evac::Params) + 8 + sizeof(evac::PolicyArgs) + sizeof(evac::NormArgs) + sizeof(evac::TransformerArgs) <= 4096,
              "k_policy_rollout_transformer: arguments beyond the kernel-argument segment");
static_assert(sizeof(evac::PolicyFamily::Smem) + sizeof(evac::PolicySmem<false>) + sizeof(evac::EvalSmem) +
                  sizeof(evac::TransformerSmem) <= 160 * 1024, "the transformer kernels' LDS beyond a CU's 160 KiB");
static_assert(sizeof(evac_transformer_block_t) == sizeof(evac::TransformerBlockArgs) && evac::kTfMaxBlocks == 2,
              "evac_transformer_block_t and the kernels' block arguments: the same 16 pointers in the same order");
static_assert(evac::kTfHeads == kTransformerHeads && evac::kTfFeedForward == kTransformerFeedForward &&
                  evac::kTfMaxModelDim == kTransformerMaxModelDim && evac::kTfMaxBlocks == kTransformerMaxBlocks &&
                  evac::kWave == kTransformerMaxTokens && evac::kTfLnEps == kTransformerLnEps,
              "evac_transformer_host.h's limits are the kernels'");

namespace {

// evac_handle_host.h's trait of an encoder.  `check` comes after the policy's thirteen tensors: what the kernels take of the
// encoder's sizes, then the handle's tokens, then the blocks' pointers and the token width (the first and the third are
// evac_transformer_host.h's, shared with the gradient's unit).
struct TransformerEncoder {
    using Struct = evac_transformer_t;
    using Args = evac::TransformerArgs;
    static constexpr const char* kRollout = "evac_policy_rollout_transformer";
    static constexpr const char* kEvaluate = "evac_policy_evaluate_transformer";
    static int check(const evac::Params& p, const evac_transformer_t& T, evac::TransformerArgs& ta, std::string& why) {
        if (const int rc = transformer_check_sizes(T, why); rc != EVAC_OK) return rc;
        if (p.n_ped + 2 > evac::kWave)
            return why = ": N = " + std::to_string(p.n_ped) + " pedestrians is not supported (one wave holds the N + 2 tokens: N <= 62)",
                   EVAC_ERR_UNSUPPORTED;
        if (p.obs_pos == EVAC_POS_GRAV) return why = ": the gravity observation is not supported (a Box observation of tokens is needed)", EVAC_ERR_UNSUPPORTED;
        if (const int rc = transformer_check_blocks(T, why); rc != EVAC_OK) return rc;
        if (T.elem_dim < 1 || T.elem_dim > evac::kTfMaxModelDim || (int64_t)T.elem_dim * (p.n_ped + 2) != (int64_t)p.obs_dim)
            return why = ": elem_dim " + std::to_string(T.elem_dim) + " x (" + std::to_string(p.n_ped) + " + 2) tokens is not the observation's " +
                         std::to_string(p.obs_dim) + " floats (a Box observation is needed)", EVAC_ERR_INVALID_ARGUMENT;
        ta = evac::TransformerArgs{};
        for (int b = 0; b < T.num_blocks; ++b) {
            const evac_transformer_block_t& B = T.blocks[b];
            ta.blk[b] = evac::TransformerBlockArgs{B.wq, B.bq, B.wk, B.bk, B.wv, B.bv, B.dense_w, B.dense_b, B.ff1_w, B.ff1_b, B.ff2_w, B.ff2_b,
                                                   B.norm1_w, B.norm1_b, B.norm2_w, B.norm2_b};
        }
        ta.elem_dim = (int)T.elem_dim;
        ta.num_blocks = (int)T.num_blocks;
        ta.use_resid = T.use_resid != 0;
        return EVAC_OK;
    }
    static auto rollout_kernel(bool norm, bool def) { return EVAC_PICK_BOOL2(evac::k_policy_rollout_transformer, norm, def); }
    static auto evaluate_kernel(bool norm, bool def) { return EVAC_PICK_BOOL2(evac::k_policy_evaluate_transformer, norm, def); }
};

}  // namespace

extern "C" {

int evac_policy_rollout_transformer(evac_handle_t h, int32_t n_steps, const evac_mlp_policy_t* policy, float* next_obs, float* next_done,
                                    float* obs_out, float* actions_out, float* logprob_out, float* value_out, float* reward_out,
                                    float* done_out, float* next_value_out, evac_episode_stats_t* final_stats, double* norm_state,
                                    float gamma, float obs_clip, float reward_clip, float epsilon, const evac_transformer_t* encoder,
                                    void* stream) {
    return encoder_rollout<TransformerEncoder>(h, n_steps, policy,
                                               collect_outputs(next_obs, next_done, obs_out, actions_out, logprob_out, value_out,
                                                               reward_out, done_out, next_value_out, final_stats),
                                               evac::NormArgs{norm_state, gamma, obs_clip, reward_clip, epsilon}, encoder, stream);
}

int evac_policy_evaluate_transformer(evac_handle_t h, int32_t agent, const evac_mlp_policy_t* policy, int32_t n_episodes,
                                     int32_t max_steps, int32_t* progress, evac_episode_stats_t* episodes_out, const double* norm_state,
                                     float obs_clip, float epsilon, const evac_transformer_t* encoder, void* stream) {
    return encoder_evaluate<TransformerEncoder>(h, agent, policy, n_episodes, max_steps, progress, episodes_out, norm_state, obs_clip,
                                                epsilon, encoder, stream);
}

}  // extern "C"
