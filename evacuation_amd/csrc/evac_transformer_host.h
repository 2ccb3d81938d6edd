// Host side of the transformer leader, the part its translation units share (evac_transformer_api.hip: collection and evaluation;
// evac_transformer_train_api.hip: the gradient; evac_transformer_update_api.hip: the optimiser step and the whole update): what the kernels take of evac_transformer_t, checked in two steps -- the sizes,
// then the blocks' pointers -- so that each entry can put its own checks (the handle's tokens, the observation's form) between
// them.  Each unit asserts the limits below against its own device constants.
#pragma once

#include <cstddef>
#include <cstdint>
#include <string>

#include "../../include/evac.h"

namespace {

constexpr int kTransformerHeads = 3;
constexpr int kTransformerFeedForward = 96;
constexpr int kTransformerMaxModelDim = 6;
constexpr int kTransformerMaxBlocks = 2;
constexpr int kTransformerMaxTokens = 64;        // one wave holds the tokens
constexpr float kTransformerLnEps = 1e-5f;

// num_heads, dim_feedforward, num_blocks, ln_eps: EVAC_ERR_UNSUPPORTED with the field named in `why`
inline int transformer_check_sizes(const evac_transformer_t& T, std::string& why) {
    if (T.num_heads != kTransformerHeads)
        return why = ": num_heads " + std::to_string(T.num_heads) + " is not supported (the kernels take 3)", EVAC_ERR_UNSUPPORTED;
    if (T.dim_feedforward != kTransformerFeedForward)
        return why = ": dim_feedforward " + std::to_string(T.dim_feedforward) + " is not supported (the kernels take 96)", EVAC_ERR_UNSUPPORTED;
    if (T.num_blocks < 1 || T.num_blocks > kTransformerMaxBlocks)
        return why = ": num_blocks " + std::to_string(T.num_blocks) + " is not supported (1 or 2)", EVAC_ERR_UNSUPPORTED;
    if (T.ln_eps != kTransformerLnEps) return why = ": ln_eps other than 1e-5 is not supported", EVAC_ERR_UNSUPPORTED;
    return EVAC_OK;
}

// The 16 pointers of a block (evac_transformer_block_t, or evac_transformer_block_grads_t: the same 16 in the same order).
template <class Block>
inline bool transformer_block_all_set(const Block& B) {
    return B.wq && B.bq && B.wk && B.bk && B.wv && B.bv && B.dense_w && B.dense_b && B.ff1_w && B.ff1_b && B.ff2_w && B.ff2_b &&
           B.norm1_w && B.norm1_b && B.norm2_w && B.norm2_b;
}
// the blocks in use (sizes checked first: num_blocks is 1 or 2): EVAC_ERR_INVALID_ARGUMENT for a NULL tensor pointer
inline int transformer_check_blocks(const evac_transformer_t& T, std::string& why) {
    for (int b = 0; b < T.num_blocks; ++b)
        if (!transformer_block_all_set(T.blocks[b]))
            return why = ": a tensor pointer of the encoder's block " + std::to_string(b) + " is NULL", EVAC_ERR_INVALID_ARGUMENT;
    return EVAC_OK;
}

// A population's encoder strides (sizes and blocks checked first): with more than one learner every stride of a block in use is
// at least its tensor; the strides of a block not in use are never looked at.  No alignment condition: the kernels read the
// encoder's tensors as scalars.
inline bool transformer_strides_ok(const evac_transformer_strides_t* st, int32_t elem_dim, int32_t num_blocks, int32_t n_learners) {
    if (n_learners <= 1) return true;
    const int64_t dm = elem_dim, H = kTransformerHeads, F = kTransformerFeedForward;
    const int64_t least[16] = {H * dm * dm, H * dm, H * dm * dm, H * dm, H * dm * dm, H * dm, dm * H * dm, dm,
                               F * dm,      F,      dm * F,      dm,     dm,          dm,     dm,          dm};
    for (int b = 0; b < num_blocks; ++b)
        for (int i = 0; i < 16; ++i)
            if ((&st->blocks[b].wq)[i] < least[i]) return false;
    return true;
}
static_assert(sizeof(evac_transformer_block_strides_t) == 16 * sizeof(int64_t) &&
                  offsetof(evac_transformer_block_strides_t, norm2_b) == 15 * sizeof(int64_t) &&
                  sizeof(evac_transformer_strides_t) == kTransformerMaxBlocks * sizeof(evac_transformer_block_strides_t),
              "transformer_strides_ok walks a block as 16 consecutive strides, wq first and norm2_b last");

}  // namespace
