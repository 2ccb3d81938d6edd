// Host side of a sweep, the part its translation units share (evac_sweep_api.hip: the linear learners;
// evac_deepsets_sweep_api.hip, evac_transformer_sweep_api.hip: behind an encoder): the learners' values from
// evac_learner_hyper_t into the kernels' arrays, and the two launches of evac_sweep_api.hip that the encoder units reuse on the
// common encoded batch, reached through plain host functions so that evac_sweep.h's kernels are defined in one translation unit
// alone (as evac_population_host.h does for the population's).
#pragma once

#include "evac_host.h"
#include "evac_learner.h"
#include "evac_sweep_args.h"

namespace evac {
// k_sweep_grad and k_sweep_finish on `stream`, and the raising of k_sweep_grad's dynamic-LDS limit (rpo_raise_lds)
void sweep_launch_grad(const RpoArgs& a, const LearnerStrides& q, const LearnerDraws& d, const LearnerLoss& h, const AdamHeader* gate,
                       dim3 grid, size_t lds, hipStream_t stream);
void sweep_launch_finish(const RpoArgs& a, const LearnerStrides& q, const LearnerDraws& d, const LearnerLoss& h, const AdamHeader* gate,
                         dim3 grid, hipStream_t stream);
int sweep_raise_grad_lds(int D, int dev);
}  // namespace evac

namespace {
// The learners' loss coefficients and optimiser values in the lone trainer's number types (`hypers`: learner_hypers_ok's)
inline void learner_values(const evac_learner_hyper_t* hypers, int32_t n_learners, evac::LearnerLoss& hl, evac::LearnerSteps& hs) {
    hl = evac::LearnerLoss{};
    hs = evac::LearnerSteps{};
    for (int s = 0; s < n_learners; ++s) {
        const evac_learner_hyper_t& y = hypers[s];
        hl.clip[s] = y.clip_coef; hl.ent[s] = y.ent_coef; hl.vf[s] = y.vf_coef; hl.alpha[s] = y.rpo_alpha;
        hs.lr[s] = y.learning_rate;
        hs.max_norm[s] = y.max_grad_norm;
        hs.target_kl[s] = y.use_target_kl ? y.target_kl : 0.0;
        if (y.use_target_kl) hs.use_target_kl |= (uint64_t)1 << s;
    }
}
}  // namespace
