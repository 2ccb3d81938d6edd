// Device code of libevac, part 13: the UPDATE of a population of transformer leaders -- S independent learners of the network of
// evac_transformer.h in the launches of one (include/evac.h: evac_transformer_update_population).
//
//   k_tf_*<const AdamHeader*, TfgLearnerStrides>   the four encoder kernels of evac_transformer_train.h with the learner as
//                                   blockIdx.y (instantiated by evac_transformer_population_update_api.hip; their lines, and what
//                                   a learner shifts and how, are there: TfgLearner, TfgMine).
//   k_adam_tf_population            k_adam_tf (evac_transformer_adam.h) with the learner as blockIdx.y: the tensor's index stays
//                                   uniform over the workgroup and the learner's shift is one scalar multiply-add on a pointer
//                                   read from the kernel-argument segment, as k_adam_set_population's.
// The three launches between the encoder's (advantage statistics, gradient, finish) are evac_population.h's, unchanged: the
// learners' encoded observations and gathered columns are laid out as ONE common batch [S][M][..] and learner s's index list is
// s M + m.  gridDim.x of every kernel is the lone kernel's, so the bodies' ticket tests (== gridDim.x - 1) hold per learner: every
// learner has its own ticket words (in its own workspace slice and header), nobody reads another learner's memory, every ticket
// is one integer atomicAdd whose result is compared, and no kernel has a loop that waits: no learner can wait on another.
#pragma once

#include "evac_transformer_adam_args.h"
#include "evac_transformer_train.h"

namespace evac {

// ---- the optimiser step: grid (wg_end[nt - 1], S); `a` as evac_transformer_update sets it (gated), learner 0's; TfAdamStrides:
// evac_transformer_adam_args.h ----
// What adam_scalars / adam_element / adam_close read of the arguments, for one learner: `a` itself stays as the launch passed it
// (a changed copy of a struct whose arrays are indexed at run time would be a private one, in scratch).
struct TfAdamLearner {
    AdamHeader* hdr;
    const float *sumsq, *stats;
    double lr, beta1, beta2, target_kl;
    float max_norm, w, b2, u, eps;
    int epoch_last, use_target_kl;
};
__global__ __launch_bounds__(kAdamBlock) void k_adam_tf_population(TfAdamArgs a, TfAdamStrides q) {
    const int64_t s = (int64_t)blockIdx.y;
    const TfAdamLearner mine{(AdamHeader*)((char*)a.hdr + s * q.hdr), a.sumsq + s * q.stats, a.stats + s * q.stats, a.lr, a.beta1, a.beta2,
                             a.target_kl, a.max_norm, a.w, a.b2, a.u, a.eps, a.epoch_last, a.use_target_kl};
    if (mine.hdr->stop) return;
    const AdamScalars k = adam_scalars(mine);
    const int b = (int)blockIdx.x, nt = a.nt;
    int i = 0;
#pragma unroll
    for (int j = 0; j < kTfAdamTensors - 1; ++j) i += (j < nt - 1 && b >= a.wg_end[j]) ? 1 : 0;
    i = __builtin_amdgcn_readfirstlane(i);      // (0 .. nt - 1 for every workgroup of the grid)
    const int first = i == 0 ? 0 : a.wg_end[i - 1];
    const int o = (b - first) * kAdamBlock + (int)threadIdx.x;
    if (o < a.n[i]) adam_element(mine, k, a.p[i] + s * q.p[i], a.g[i] + s * q.g[i], a.m[i] + s * q.m[i], a.v[i] + s * q.m[i], o);
    adam_close(mine, k);
}

}  // namespace evac
