// Device code of libevac, part 8: a population whose learners differ in their hyperparameters (include/evac.h:
// evac_gae_learners, evac_rpo_update_sweep; the collection's sibling, k_collect_sweep, is evac_policy.h's).  The values travel
// as the learners' seeds do (evac_learner.h: LearnerDraws): arrays by value in the kernel-argument segment, read at the learner's
// index.  In the update's kernels that index comes from the block index, so the read is a scalar load from the segment and the
// learner's argument struct is the population's with four (gradient, finish) or four (optimiser) fields overwritten; the body
// each kernel runs is the one-learner kernel's.  The lone trainer's number types are kept so that the bits match: lr and
// target_kl double, the loss coefficients and max_grad_norm float32, gamma and gamma x lambda float32 (rounded on the host).
#pragma once

#include "evac_learner.h"
#include "evac_sweep_args.h"                    // LearnerLoss, LearnerSteps, LearnerDiscounts

namespace evac {

__device__ __forceinline__ RpoArgs learner_loss_args(RpoArgs a, const LearnerLoss& h, int s) {
    a.clip = h.clip[s]; a.ent = h.ent[s]; a.vf = h.vf[s]; a.alpha = h.alpha[s];
    return a;
}

// k_gae (evac_train_api.hip) with the learner's pair: env e is learner e / E_l's.  A learner's boundary may fall inside a wave,
// so the pair is read per lane.  The arithmetic is k_gae's, operation for operation.  TWIN: change one, change the other (a shared
// body changes both kernels' instructions: DESIGN.md section 4.11); likewise the three kernels below and evac_population.h's.
__global__ __launch_bounds__(256) void k_sweep_advantages(int T, int64_t E, const float* __restrict__ rewards,
                                                          const float* __restrict__ values, const float* __restrict__ dones,
                                                          const float* __restrict__ next_value, const float* __restrict__ next_done,
                                                          int64_t envs_per_learner, LearnerDiscounts h, float* __restrict__ adv_out,
                                                          float* __restrict__ ret_out) {
    const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (e >= E) return;
    int s = (int)(e / envs_per_learner);
    s = s < kMaxLearners ? s : kMaxLearners - 1;       // (the host checked E = S E_l: never taken)
    const float gamma = h.gamma[s], gl = h.gl[s];
    float vn = next_value[e], dn = next_done[e], last = 0.0f;
    for (int t = T - 1; t >= 0; --t) {
        const size_t i = (size_t)t * (size_t)E + (size_t)e;
        const float r = rewards[i], v = values[i], d = dones[i];
        const float nonterminal = __fsub_rn(1.0f, dn);
        const float delta = __fsub_rn(__fadd_rn(r, __fmul_rn(__fmul_rn(gamma, vn), nonterminal)), v);
        last = __fadd_rn(delta, __fmul_rn(__fmul_rn(gl, nonterminal), last));
        adv_out[i] = last;
        ret_out[i] = __fadd_rn(last, v);
        vn = v;
        dn = d;
    }
}

// grid (P, 2, S): k_population_grad with the learner's clip / ent / vf / alpha (TWIN of it)
__global__ __launch_bounds__(kGradBlock) void k_sweep_grad(RpoArgs a, LearnerStrides q, LearnerDraws d, LearnerLoss h,
                                                           const AdamHeader* gate) {
    extern __shared__ __attribute__((aligned(16))) float sweep_lds[];
    const int s = (int)blockIdx.z;
    if (rpo_stopped(learner_header(gate, q, s))) return;
    const RpoArgs la = learner_loss_args(learner_rpo_args(a, q, d, s), h, s);
    rpo_clear_tickets(la.ws);
    if (blockIdx.y == 0) rpo_grad_body<true>(la, sweep_lds);
    else rpo_grad_body<false>(la, sweep_lds);
}
// grid (10 + 2 x tiles x segments, S): k_population_finish with the learner's coefficients (the body reads ent and vf: the
// entropy's gradient of logstd and the logged loss).  TWIN of k_population_finish.
__global__ __launch_bounds__(kFinishBlock) void k_sweep_finish(RpoArgs a, LearnerStrides q, LearnerDraws d, LearnerLoss h,
                                                               const AdamHeader* gate) {
    __shared__ RpoArgs mine;
    const int s = (int)blockIdx.y;
    if (rpo_stopped(learner_header(gate, q, s))) return;
    if (threadIdx.x == 0) mine = learner_loss_args(learner_rpo_args(a, q, d, s), h, s);
    __syncthreads();
    rpo_finish_body<const RpoArgs&>(mine);
}
// grid (ceil(elements / 256), S): k_population_optimizer with the learner's lr, max_norm and target (TWIN of it)
__global__ __launch_bounds__(kAdamBlock) void k_sweep_optimizer(AdamArgs a, LearnerStrides q, LearnerSteps h) {
    __shared__ AdamArgs mine;
    const int s = (int)blockIdx.y, t = (int)threadIdx.x;
    AdamHeader* hdr = (AdamHeader*)((char*)a.hdr + s * q.hdr);
    if (hdr->stop) return;
    if (t < kAdamTensors) {
        mine.p[t] = a.p[t] + s * q.p[t];
        mine.g[t] = a.g[t] + s * q.g[t];
        mine.m[t] = a.m[t] + s * q.m[t];
        mine.v[t] = a.v[t] + s * q.m[t];
        mine.end[t] = a.end[t];
    } else if (t == 64) {
        mine.hdr = hdr;
        mine.sumsq = a.sumsq + s * q.stats;
        mine.stats = a.stats + s * q.stats;
        mine.lr = h.lr[s]; mine.beta1 = a.beta1; mine.beta2 = a.beta2; mine.target_kl = h.target_kl[s];
        mine.max_norm = h.max_norm[s]; mine.w = a.w; mine.b2 = a.b2; mine.u = a.u; mine.eps = a.eps;
        mine.gated = a.gated; mine.epoch_last = a.epoch_last; mine.use_target_kl = (int)((h.use_target_kl >> s) & 1u);
    }
    __syncthreads();
    adam_stage(mine);
}

}  // namespace evac
