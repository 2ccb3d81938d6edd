// Device code of libevac, part 9: the DEEP-SETS LEADER'S OPTIMISER STEP -- clip_grad_norm_ and Adam of evac_train.h (k_adam) for
// the network of evac_deepsets.h: the 13 tensors of evac_mlp_policy_grads_t followed by the 6 of evac_deepsets_grads_t, one launch,
// one clip coefficient, one step count, one header (include/evac.h: evac_deepsets_adam_step).
//
// The contract is k_adam's in every point, and the arithmetic is k_adam's code: adam_scalars, adam_element and adam_close of
// evac_train.h.  What differs is how a thread finds its tensor.  k_adam numbers the elements of all tensors in one run and picks
// the tensor per lane with a chain of 12 compare-selects over 4 x 13 pointers; 18 of them over 4 x 19 do not fit the scalar
// registers (36 bytes of scratch per lane, 4 spilled SGPRs: measured).  Here every tensor starts at a WORKGROUP boundary:
// wg_end[i] is the running count of ceil(n_i / 256), the grid is wg_end[18] (at most 18 part-filled workgroups), the tensor's
// index is counted from blockIdx.x against wg_end[] -- uniform over the workgroup -- and indexes the pointer arrays of the
// by-value argument struct directly: scalar loads from the kernel-argument segment, no select chain, no private copy.
#pragma once

#include "evac_deepsets_adam_args.h"
#include "evac_train.h"

namespace evac {

__global__ __launch_bounds__(kAdamBlock) void k_adam_set(SetAdamArgs a) {
    if (a.gated && a.hdr->stop) return;
    const AdamScalars k = adam_scalars(a);
    const int b = (int)blockIdx.x;
    int i = 0;
#pragma unroll
    for (int j = 0; j < kSetAdamTensors - 1; ++j) i += b >= a.wg_end[j] ? 1 : 0;
    i = __builtin_amdgcn_readfirstlane(i);      // (0 .. 18 for every workgroup of the grid)
    const int first = i == 0 ? 0 : a.wg_end[i - 1];
    const int o = (b - first) * kAdamBlock + (int)threadIdx.x;
    if (o < a.n[i]) adam_element(a, k, a.p[i], a.g[i], a.m[i], a.v[i], o);
    adam_close(a, k);
}

}  // namespace evac
