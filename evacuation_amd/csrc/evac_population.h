// Device code of libevac, part 7: the trainer's update for a POPULATION -- S independent learners of one configuration in the
// launches of one (include/evac.h: evac_rpo_update_population).  The four kernels of a minibatch step (evac_train.h) with the
// learner as one more grid dimension: a workgroup shifts the argument struct by its learner's strides -- parameters, gradients,
// moments, header, workspace slice, index list, statistics row, noise row, seed and draw counter -- and runs the body the
// one-learner kernel runs.  gridDim.x is the one-learner kernel's, so the bodies' ticket tests (== gridDim.x - 1) hold per learner:
// every learner has its own ticket words (in its own workspace slice and header) and nobody reads another learner's memory, so
// no learner can wait on another.  A learner whose stop flag is set returns at once; the others go on.
#pragma once

#include "evac_learner.h"
#include "evac_train.h"

namespace evac {

// every learner's stop, steps_run, epochs_run (and the ticket, zero anyway) before the call's first step: one thread per learner
__global__ __launch_bounds__(kMaxLearners) void k_population_begin(AdamHeader* h, int64_t stride, int n_learners) {
    const int s = (int)threadIdx.x;
    if (s >= n_learners) return;
    AdamHeader* mine = (AdamHeader*)((char*)h + s * stride);
    mine->stop = 0;
    mine->steps_run = 0;
    mine->epochs_run = 0;
    mine->ticket = 0u;
}
// grid (1, S)
__global__ __launch_bounds__(kFinishBlock) void k_population_adv_stats(RpoArgs a, LearnerStrides q, LearnerDraws d, const AdamHeader* gate) {
    __shared__ double buf[kFinishBlock];
    const int s = (int)blockIdx.y;
    if (rpo_stopped(learner_header(gate, q, s))) return;
    rpo_adv_stats_body(learner_rpo_args(a, q, d, s), buf);
}
// grid (P, 2, S).  TWIN: k_sweep_grad (evac_sweep.h) repeats these lines; change one, change the other
__global__ __launch_bounds__(kGradBlock) void k_population_grad(RpoArgs a, LearnerStrides q, LearnerDraws d, const AdamHeader* gate) {
    extern __shared__ __attribute__((aligned(16))) float population_lds[];
    const int s = (int)blockIdx.z;
    if (rpo_stopped(learner_header(gate, q, s))) return;
    const RpoArgs la = learner_rpo_args(a, q, d, s);
    rpo_clear_tickets(la.ws);
    if (blockIdx.y == 0) rpo_grad_body<true>(la, population_lds);
    else rpo_grad_body<false>(la, population_lds);
}
// grid (10 + 2 x tiles x segments, S).  The finishing body picks its net's pointers at run time (a.net[net]): the learner's
// arguments are formed once, by thread 0, and lie in LDS -- registers cannot be indexed, and a private copy would be scratch.
// TWIN: k_sweep_finish (evac_sweep.h); change one, change the other.
__global__ __launch_bounds__(kFinishBlock) void k_population_finish(RpoArgs a, LearnerStrides q, LearnerDraws d, const AdamHeader* gate) {
    __shared__ RpoArgs mine;
    const int s = (int)blockIdx.y;
    if (rpo_stopped(learner_header(gate, q, s))) return;
    if (threadIdx.x == 0) mine = learner_rpo_args(a, q, d, s);
    __syncthreads();
    rpo_finish_body<const RpoArgs&>(mine);
}
// grid (ceil(elements / 256), S); `a` as evac_rpo_update sets it (gated), sumsq / stats pointing into learner 0's statistics row.
// The learner's 4 x 13 pointers are formed by 13 threads and lie in LDS: adam_stage picks a thread's tensor with per-lane
// selects, so they end in vector registers either way, and 52 shifted pointers at once would not fit the scalar registers.
// TWIN: k_sweep_optimizer (evac_sweep.h); change one, change the other.
__global__ __launch_bounds__(kAdamBlock) void k_population_optimizer(AdamArgs a, LearnerStrides q) {
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
        mine.lr = a.lr; mine.beta1 = a.beta1; mine.beta2 = a.beta2; mine.target_kl = a.target_kl;
        mine.max_norm = a.max_norm; mine.w = a.w; mine.b2 = a.b2; mine.u = a.u; mine.eps = a.eps;
        mine.gated = a.gated; mine.epoch_last = a.epoch_last; mine.use_target_kl = a.use_target_kl;
    }
    __syncthreads();
    adam_stage(mine);
}

}  // namespace evac
