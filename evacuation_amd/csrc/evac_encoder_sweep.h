// Device code of libevac, part 14: what the sweeps of the two encoder leaders share (include/evac.h: evac_deepsets_update_sweep,
// evac_transformer_update_sweep; the units' own kernels are in evac_deepsets_sweep_api.hip and evac_transformer_sweep_api.hip).
//
// Where the optimiser's values travel.  The loss coefficients ride by value as the linear sweep's do (LearnerLoss into
// k_sweep_grad / k_sweep_finish, on the common encoded batch).  The optimiser's do not fit beside the transformer's arguments
// (TfAdamArgs + TfAdamStrides + LearnerSteps is past the 4 KiB of the kernel-argument segment), so for both encoders one launch
// per update call copies the by-value LearnerSteps into a table at the workspace's tail (k_learner_steps_table) and the
// optimiser's kernels read their learner's entry from there: blockIdx.y is the learner, so the address is uniform over the
// workgroup and the reads are scalar loads.  The table is written once per call and only read behind it, in stream order: the
// call stays capturable and free of host copies, and a capture freezes the values as it freezes the seeds.
// Only templates here, so more than one translation unit may include this header.
#pragma once

#include "evac_sweep_args.h"
#include "evac_train.h"

namespace evac {

constexpr int kStepsTableBlock = 64;
constexpr int kStepsTableWords = (int)(sizeof(LearnerSteps) / sizeof(uint32_t));
static_assert(sizeof(LearnerSteps) % sizeof(uint32_t) == 0, "k_learner_steps_table copies whole 32-bit words");

// grid (1), one wave: the table is LearnerSteps as the host filled it, word for word.  UNIT names the translation unit (a
// plain __global__ in a header that two units include would be defined twice at link).
template <int UNIT>
__global__ __launch_bounds__(kStepsTableBlock) void k_learner_steps_table(LearnerSteps h, LearnerSteps* __restrict__ table) {
    const uint32_t* src = (const uint32_t*)&h;
    uint32_t* dst = (uint32_t*)table;
    for (int i = (int)threadIdx.x; i < kStepsTableWords; i += kStepsTableBlock) dst[i] = src[i];
}

// What adam_scalars / adam_element / adam_close read of the arguments, for one learner of a sweep: SetAdamLearner's /
// TfAdamLearner's fields (evac_deepsets_population.h, evac_transformer_population_train.h), of which lr, target_kl, max_norm and
// use_target_kl come from the learner's entry of the table.
struct SweepAdamLearner {
    AdamHeader* hdr;
    const float *sumsq, *stats;
    double lr, beta1, beta2, target_kl;
    float max_norm, w, b2, u, eps;
    int epoch_last, use_target_kl;
};
template <class Args, class Strides>
__device__ __forceinline__ SweepAdamLearner sweep_adam_learner(const Args& a, const Strides& q, const LearnerSteps* __restrict__ h,
                                                               int64_t s) {
    return SweepAdamLearner{(AdamHeader*)((char*)a.hdr + s * q.hdr), a.sumsq + s * q.stats, a.stats + s * q.stats, h->lr[s], a.beta1,
                            a.beta2, h->target_kl[s], h->max_norm[s], a.w, a.b2, a.u, a.eps, a.epoch_last,
                            (int)((h->use_target_kl >> s) & 1u)};
}

}  // namespace evac
