// Host side of the transformer leader, the part the units that run it on a handle's envs share (evac_transformer_api.hip:
// collection and evaluation; evac_capture_api.hip: the recording evaluation): the attention encoder against the handle, as
// evac_handle_host.h's trait of an encoder asks for it.  A unit derives its trait from this and adds its entries' names and
// kernels.  (evac_transformer_host.h is the part that the gradient's unit shares too: it knows no handle.)
#pragma once

#include <cstdint>
#include <cstring>
#include <string>

#include "evac_transformer.h"
#include "evac_transformer_population.h"       // (TransformerStrides; its kernel templates are instantiated by their own units)
#include "evac_handle_host.h"
#include "evac_transformer_host.h"

static_assert(sizeof(evac_transformer_block_t) == sizeof(evac::TransformerBlockArgs) && evac::kTfMaxBlocks == 2,
              "evac_transformer_block_t and the kernels' block arguments: the same 16 pointers in the same order");
static_assert(sizeof(evac_transformer_block_strides_t) == sizeof(evac::TransformerBlockStrides),
              "evac_transformer_block_strides_t and the kernels' block strides: the same 16 strides in the same order");
static_assert(evac::kTfHeads == kTransformerHeads && evac::kTfFeedForward == kTransformerFeedForward &&
                  evac::kTfMaxModelDim == kTransformerMaxModelDim && evac::kTfMaxBlocks == kTransformerMaxBlocks &&
                  evac::kWave == kTransformerMaxTokens && evac::kTfLnEps == kTransformerLnEps,
              "evac_transformer_host.h's limits are the kernels'");

namespace evac {
// k_collect_population_transformer on `stream` (evac_transformer_population_api.hip; the sweep's unit launches it on a raw env,
// where no gamma enters collection): a plain host function, so that the kernel is instantiated in one translation unit alone
void transformer_population_launch_collect(const evac_host::HandleView& v, int n_steps, const PolicyArgs& a, const NormArgs& na,
                                           int n_learners, const PopulationArgs& q, const TransformerArgs& ea,
                                           const TransformerStrides& tq, hipStream_t stream);
}  // namespace evac

namespace {

// `check` comes after the policy's thirteen tensors: what the kernels take of the encoder's sizes, then the handle's tokens, then
// the blocks' pointers and the token width (the first and the third are evac_transformer_host.h's).
struct TransformerEncoderHost {
    using Struct = evac_transformer_t;
    using Args = evac::TransformerArgs;
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
};

// The learners of a population of such networks, for evac_handle_host.h's Learners of encoder_rollout / encoder_evaluate
// (evac_transformer_population_api.hip, evac_transformer_population_evaluate_api.hip): their shares of the handle's envs and the
// strides of their 13 + 16 num_blocks tensors, refused behind the networks.  A unit derives its Learners from this and adds its
// launch.
struct TransformerLearnerShares {
    static constexpr bool kOn = true;
    int32_t n_learners;
    const evac_mlp_policy_strides_t* strides;
    const evac_transformer_strides_t* enc_strides;
    evac::PopulationArgs q{};
    evac::TransformerStrides tq{};

    std::string check(const evac::Params& p, const evac_mlp_policy_t& policy, const evac_transformer_t& encoder) {
        std::string why = learner_shares(p.n_envs, n_learners, strides, policy.obs_dim, q);
        if (!why.empty()) return why;
        if (!transformer_strides_ok(enc_strides, encoder.elem_dim, encoder.num_blocks, n_learners))
            return ": an encoder stride of a block in use is smaller than its tensor";
        for (int b = 0; b < encoder.num_blocks; ++b) std::memcpy(&tq.blk[b], &enc_strides->blocks[b], sizeof tq.blk[b]);
        return why;
    }
};

}  // namespace
