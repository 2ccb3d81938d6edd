// Device code of libevac: what the kernels of a population share (evac_population.h: one configuration; evac_sweep.h: a
// configuration per learner) -- a learner's strides, its seed and draw counter, and the shift of the one-learner argument
// struct to learner s.  No kernel is defined here, so more than one translation unit may include this header.
#pragma once

#include "evac_train.h"

namespace evac {

struct LearnerStrides {
    int64_t p[kAdamTensors], g[kAdamTensors], m[kAdamTensors];   // floats: parameters, gradients, moments (both of them)
    int64_t hdr, ws;                            // bytes
    int64_t inds, stats, noise;                 // elements of perms / stats_out / rpo_noise per learner
};
struct LearnerDraws {                           // by value: 1 KiB of kernel arguments
    uint64_t seed[kMaxLearners], first_counter[kMaxLearners];
};

__device__ __forceinline__ const AdamHeader* learner_header(const AdamHeader* h, const LearnerStrides& q, int s) {
    return (const AdamHeader*)((const char*)h + s * q.hdr);
}
// RpoArgs of learner s.  `a` holds learner 0's pointers and, as its draw counter, the step's number in the call.
__device__ __forceinline__ RpoArgs learner_rpo_args(RpoArgs a, const LearnerStrides& q, const LearnerDraws& d, int s) {
#pragma unroll
    for (int n = 0; n < 2; ++n) {
        const int o = 7 * n;
        RpoNet& t = a.net[n];
        t.w1 += s * q.p[o]; t.b1 += s * q.p[o + 1]; t.w2 += s * q.p[o + 2]; t.b2 += s * q.p[o + 3]; t.w3 += s * q.p[o + 4]; t.b3 += s * q.p[o + 5];
        t.gw1 += s * q.g[o]; t.gb1 += s * q.g[o + 1]; t.gw2 += s * q.g[o + 2]; t.gb2 += s * q.g[o + 3]; t.gw3 += s * q.g[o + 4]; t.gb3 += s * q.g[o + 5];
    }
    a.logstd += s * q.p[6];
    a.glogstd += s * q.g[6];
    a.inds += s * q.inds;
    if (a.noise) a.noise += s * q.noise;
    a.stats += s * q.stats;
    a.ws += s * q.ws;
    const uint64_t ctr = d.first_counter[s] + (((uint64_t)a.ctr_hi << 32) | a.ctr_lo), seed = d.seed[s];
    a.seed_lo = (uint32_t)seed; a.seed_hi = (uint32_t)(seed >> 32);
    a.ctr_lo = (uint32_t)ctr; a.ctr_hi = (uint32_t)(ctr >> 32);
    return a;
}

}  // namespace evac
