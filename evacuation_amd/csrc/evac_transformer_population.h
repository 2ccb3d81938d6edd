// Device code of libevac, part 12: a POPULATION of transformer leaders on a handle's envs -- S independent learners of the
// network of evac_transformer.h in one launch (include/evac.h: evac_policy_rollout_population_transformer,
// evac_policy_evaluate_population_transformer).
//
//   k_collect_population_transformer    k_collect_population_deepsets' lines (evac_deepsets_population.h) with the attention
//                                       encoder: learner s owns envs [s E_l, (s + 1) E_l) and ceil(E_l / 16) workgroups.
//   k_evaluate_population_transformer   k_evaluate_population_deepsets' lines (evac_deepsets_population_evaluate.h) likewise.
// A workgroup never mixes learners, so the encoder's staging of both blocks' weights in LDS (TransformerEncoderOf::stage, once per
// workgroup) is per learner as it stands and the shifts need no LDS.
//
// The learner's shift.  stage() takes its block's 16 pointers from the kernel-argument segment with a run-time block index; a
// changed private copy of TransformerArgs would be indexed at run time too and go to scratch (evac_deepsets_population.h records
// 856 bytes for the optimiser's), and so does a shifted copy of one block's 16 pointers (48 bytes measured: the six vectors'
// pointers, chosen per thread, became a table).  So the arguments stay as the launch passed them and stage() asks
// TransformerLearnerTensors::of for each tensor where it names it: the pointer and its stride are scalar loads from the
// kernel-argument segment, the shift one scalar multiply-add, and no array exists.  Nothing waits across workgroups.
#pragma once

#include "evac_transformer.h"

namespace evac {

// floats from learner s to learner s + 1, per tensor of evac_transformer_block_t, in its order
struct TransformerBlockStrides {
    int64_t wq, bq, wk, bk, wv, bv, dense_w, dense_b, ff1_w, ff1_b, ff2_w, ff2_b, norm1_w, norm1_b, norm2_w, norm2_b;
};
struct TransformerStrides {
    TransformerBlockStrides blk[kTfMaxBlocks];
};

static_assert(sizeof(TransformerBlockStrides) == kTfBlockTensors * sizeof(int64_t), "a stride per TransformerTensor, in its order");

// Learner s's tensors for TransformerEncoderOf::stage: tensor i of block b, s strides further.  (i is a constant where stage()
// names a tensor, so the stride is one scalar load at a fixed offset behind the block's run-time one.)
struct TransformerLearnerTensors {
    const TransformerStrides& tq;
    int s;
    __device__ __forceinline__ const float* of(const float* tensor, int b, int i) const { return tensor + s * (&tq.blk[b].wq)[i]; }
    // encode()'s lane and row, opaque to the compiler.  The step body is at the limit of 128 registers and the loop-invariant LDS
    // addresses that encode() forms from the two were carried through the step loop: with the learner's scalars beside them
    // three of the eight kernels spilled one or two registers to scratch (8 B, 8 B, 12 B measured).  An empty asm makes the
    // compiler form those addresses at every call (and the k, v address for every channel): no spill and no scratch in any of
    // the eight, for 10 -- 12 % more time per step than the lone kernels.
    static constexpr bool kFresh = true;
    static __device__ __forceinline__ int fresh(int v) {
        asm volatile("" : "+v"(v));
        return v;
    }
    static __device__ __forceinline__ float* fresh(float* v) {
        auto lds = (__attribute__((address_space(3))) float*)v;          // (the wave's row of PolicySmem::x: the address stays an LDS one)
        asm volatile("" : "+v"(lds));
        return (float*)lds;
    }
};
using TransformerLearnerEncoder = TransformerEncoderOf<TransformerLearnerTensors>;

// ---- collection ----
template <bool NORM, bool DEF>
__global__ __launch_bounds__(PolicyFamily::kBlock, 4) void k_collect_population_transformer(Params p, int n_steps, PolicyArgs a, NormArgs na,
                                                                                             PopulationArgs q, TransformerArgs ta,
                                                                                             TransformerStrides tq) {
    __shared__ PolicyFamily::Smem sm;
    __shared__ PolicySmem<false> ps;
    __shared__ TransformerSmem ts;
    if constexpr (DEF) p = default_config_constants<false>(p);
    const int s = (int)blockIdx.x / q.wgs;
    const PolicyArgs la = learner_policy(a, q, s);
    // (blockIdx.x x 16 + slot) + shift = s E_l + (blockIdx.x - s wgs) x 16 + slot
    policy_rollout_body<false, NORM, true, TransformerLearnerEncoder>(sm, ps, p, n_steps, la, na,
                                                                      s * (q.envs_per_learner - q.wgs * PolicyFamily::kEnvsPerBlock),
                                                                      (s + 1) * q.envs_per_learner,
                                                                      TransformerLearnerEncoder{ts, ta, {tq, s}});
}

// ---- evaluation: progress, episodes_out and norm_state are indexed by the handle's env.  shared != 0: learner s's env i draws
// with the id of env i, whoever the learner is ----
template <bool NORM, bool DEF>
__global__ __launch_bounds__(PolicyFamily::kBlock, 4) void k_evaluate_population_transformer(Params p, PolicyArgs a, EvalArgs ev,
                                                                                              PopulationArgs q, TransformerArgs ta,
                                                                                              TransformerStrides tq, int shared) {
    __shared__ PolicyFamily::Smem sm;
    __shared__ PolicySmem<false> ps;
    __shared__ EvalSmem es;
    __shared__ TransformerSmem ts;
    if constexpr (DEF) p = default_config_constants<false>(p);
    const int s = (int)blockIdx.x / q.wgs;
    const PolicyArgs la = learner_policy(a, q, s);
    // (blockIdx.x x 16 + slot) + shift = s E_l + (blockIdx.x - s wgs) x 16 + slot
    policy_evaluate_body<true, false, NORM, TransformerLearnerEncoder, true>(
        sm, &ps, es, p, la, ev, TransformerLearnerEncoder{ts, ta, {tq, s}}, s * (q.envs_per_learner - q.wgs * PolicyFamily::kEnvsPerBlock),
        (s + 1) * q.envs_per_learner, shared ? s * q.envs_per_learner : 0);
}

}  // namespace evac
