// Device code of libevac, part 11: the EVALUATION of a population of deep-sets leaders -- every learner's whole episodes in one
// launch (include/evac.h: evac_policy_evaluate_population_deepsets).
//
//   k_evaluate_population_deepsets  k_evaluate_population's lines (evac_evaluate.h) with DeepSetsEncoder: learner s owns envs
//                                   [s E_l, (s + 1) E_l) of the handle and ceil(E_l / 16) workgroups of the launch, stages its own
//                                   13 + 6 tensors (the encoder's pointers moved as k_collect_population_deepsets moves them) and
//                                   runs policy_evaluate_body on its envs.  A workgroup never mixes learners, so the encoder's
//                                   staging of W_a, W_b, b_b in LDS is per learner as it stands, and the shifts need no LDS.
// progress, episodes_out and norm_state are indexed by the handle's env.  shared != 0: learner s's env i draws with the id of env
// i, whoever the learner is.  Nothing waits across workgroups: a learner's envs end when they end.
#pragma once

#include "evac_deepsets.h"

namespace evac {

template <bool NORM, bool DEF>
__global__ __launch_bounds__(PolicyFamily::kBlock, 4) void k_evaluate_population_deepsets(Params p, PolicyArgs a, EvalArgs ev,
                                                                                           PopulationArgs q, DeepSetsArgs da,
                                                                                           DeepSetsStrides dq, int shared) {
    __shared__ PolicyFamily::Smem sm;
    __shared__ PolicySmem<false> ps;
    __shared__ EvalSmem es;
    __shared__ DeepSetsSmem ds;
    if constexpr (DEF) p = default_config_constants<false>(p);
    const int s = (int)blockIdx.x / q.wgs;
    const PolicyArgs la = learner_policy(a, q, s);
    da.phi_w1 += s * dq.stride[0]; da.phi_b1 += s * dq.stride[1]; da.phi_w2 += s * dq.stride[2]; da.phi_b2 += s * dq.stride[3];
    da.rho_w += s * dq.stride[4]; da.rho_b += s * dq.stride[5];
    // (blockIdx.x x 16 + slot) + shift = s E_l + (blockIdx.x - s wgs) x 16 + slot
    policy_evaluate_body<true, false, NORM, DeepSetsEncoder, true>(sm, &ps, es, p, la, ev, DeepSetsEncoder{ds, da},
                                                                   s * (q.envs_per_learner - q.wgs * PolicyFamily::kEnvsPerBlock),
                                                                   (s + 1) * q.envs_per_learner, shared ? s * q.envs_per_learner : 0);
}

}  // namespace evac
