// Device code of libevac, part 10: a POPULATION of deep-sets leaders -- S independent learners of the network of evac_deepsets.h
// in the launches of one (include/evac.h: evac_policy_rollout_population_deepsets, evac_deepsets_update_population).
//
//   k_collect_population_deepsets   k_collect_population's lines (evac_policy.h) with DeepSetsEncoder: learner s owns envs
//                                   [s E_l, (s + 1) E_l) and ceil(E_l / 16) workgroups; a workgroup never mixes learners, so the
//                                   encoder's staging of W_a, W_b, b_b in LDS is per learner as it stands.
//   k_set_*<const AdamHeader*, SetLearnerStrides>    the three encoder kernels of evac_deepsets_train.h with the learner as
//                                   blockIdx.y (instantiated by evac_deepsets_population_api.hip; their lines are there).
//   k_adam_set_population           k_adam_set (evac_deepsets_adam.h) with the learner as blockIdx.y: the tensor's index stays
//                                   uniform over the workgroup and the learner's shift is one scalar multiply-add on a pointer
//                                   read from the kernel-argument segment.
// The three launches between the encoder's (advantage statistics, gradient, finish) are evac_population.h's, unchanged: the
// learners' encoded observations and gathered columns are laid out as ONE common batch [S][M][..] and learner s's index list is
// s M + m.  gridDim.x of every kernel is the lone kernel's, so the bodies' ticket tests (== gridDim.x - 1) hold per learner: every
// learner has its own ticket words (in its own workspace slice and header), nobody reads another learner's memory, every ticket
// is one integer atomicAdd whose result is compared, and no kernel has a loop that waits: no learner can wait on another.
#pragma once

#include "evac_deepsets.h"
#include "evac_deepsets_adam_args.h"
#include "evac_deepsets_train.h"

namespace evac {

// ---- collection (DeepSetsStrides: evac_deepsets.h) ----
template <bool NORM, bool DEF>
__global__ __launch_bounds__(PolicyFamily::kBlock, 4) void k_collect_population_deepsets(Params p, int n_steps, PolicyArgs a, NormArgs na,
                                                                                          PopulationArgs q, DeepSetsArgs da,
                                                                                          DeepSetsStrides dq) {
    __shared__ PolicyFamily::Smem sm;
    __shared__ PolicySmem<false> ps;
    __shared__ DeepSetsSmem ds;
    if constexpr (DEF) p = default_config_constants<false>(p);
    const int s = (int)blockIdx.x / q.wgs;
    const PolicyArgs la = learner_policy(a, q, s);
    da.phi_w1 += s * dq.stride[0]; da.phi_b1 += s * dq.stride[1]; da.phi_w2 += s * dq.stride[2]; da.phi_b2 += s * dq.stride[3];
    da.rho_w += s * dq.stride[4]; da.rho_b += s * dq.stride[5];
    // (blockIdx.x x 16 + slot) + shift = s E_l + (blockIdx.x - s wgs) x 16 + slot
    policy_rollout_body<false, NORM, true, DeepSetsEncoder>(sm, ps, p, n_steps, la, na,
                                                            s * (q.envs_per_learner - q.wgs * PolicyFamily::kEnvsPerBlock),
                                                            (s + 1) * q.envs_per_learner, DeepSetsEncoder{ds, da});
}

// ---- the optimiser step: grid (wg_end[18], S); `a` as evac_deepsets_update sets it (gated), learner 0's; SetAdamStrides:
// evac_deepsets_adam_args.h ----
// What adam_scalars / adam_element / adam_close read of the arguments, for one learner: `a` itself stays as the launch passed it
// (a changed copy of a struct whose arrays are indexed at run time would be a private one: 856 bytes of scratch, measured).
struct SetAdamLearner {
    AdamHeader* hdr;
    const float *sumsq, *stats;
    double lr, beta1, beta2, target_kl;
    float max_norm, w, b2, u, eps;
    int epoch_last, use_target_kl;
};
__global__ __launch_bounds__(kAdamBlock) void k_adam_set_population(SetAdamArgs a, SetAdamStrides q) {
    const int64_t s = (int64_t)blockIdx.y;
    const SetAdamLearner mine{(AdamHeader*)((char*)a.hdr + s * q.hdr), a.sumsq + s * q.stats, a.stats + s * q.stats, a.lr, a.beta1, a.beta2,
                              a.target_kl, a.max_norm, a.w, a.b2, a.u, a.eps, a.epoch_last, a.use_target_kl};
    if (mine.hdr->stop) return;
    const AdamScalars k = adam_scalars(mine);
    const int b = (int)blockIdx.x;
    int i = 0;
#pragma unroll
    for (int j = 0; j < kSetAdamTensors - 1; ++j) i += b >= a.wg_end[j] ? 1 : 0;
    i = __builtin_amdgcn_readfirstlane(i);      // (0 .. 18 for every workgroup of the grid)
    const int first = i == 0 ? 0 : a.wg_end[i - 1];
    const int o = (b - first) * kAdamBlock + (int)threadIdx.x;
    if (o < a.n[i]) adam_element(mine, k, a.p[i] + s * q.p[i], a.g[i] + s * q.g[i], a.m[i] + s * q.m[i], a.v[i] + s * q.m[i], o);
    adam_close(mine, k);
}

}  // namespace evac
