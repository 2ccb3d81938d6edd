// Device code of libevac, part 10: the TRANSFORMER LEADER'S OPTIMISER STEP -- clip_grad_norm_ and Adam of evac_train.h (k_adam)
// for the network of evac_transformer.h: the 13 tensors of evac_mlp_policy_grads_t followed by the 16 of every block in use in
// evac_transformer_block_grads_t order, blocks[0] first -- 29 tensors with one block, 45 with two -- one launch, one clip
// coefficient, one step count, one header (include/evac.h: evac_transformer_adam_step).
//
// The scheme is k_adam_set's (evac_deepsets_adam.h) with the number of tensors a runtime field: every tensor starts at a
// WORKGROUP boundary, wg_end[i] is the running count of ceil(n_i / 256), the grid is wg_end[nt - 1], the tensor's index is
// counted from blockIdx.x against wg_end[] -- uniform over the workgroup -- and indexes the pointer arrays of the by-value
// argument struct directly: scalar loads from the kernel-argument segment, no select chain, no private copy.  The entries of a
// block that is not in use are never looked at: the count stops at nt.  The arithmetic is k_adam's code: adam_scalars,
// adam_element and adam_close of evac_train.h.
#pragma once

#include "evac_transformer_adam_args.h"
#include "evac_train.h"

namespace evac {

__global__ __launch_bounds__(kAdamBlock) void k_adam_tf(TfAdamArgs a) {
    if (a.gated && a.hdr->stop) return;
    const AdamScalars k = adam_scalars(a);
    const int b = (int)blockIdx.x, nt = a.nt;
    int i = 0;
#pragma unroll
    for (int j = 0; j < kTfAdamTensors - 1; ++j) i += (j < nt - 1 && b >= a.wg_end[j]) ? 1 : 0;
    i = __builtin_amdgcn_readfirstlane(i);      // (0 .. nt - 1 for every workgroup of the grid)
    const int first = i == 0 ? 0 : a.wg_end[i - 1];
    const int o = (b - first) * kAdamBlock + (int)threadIdx.x;
    if (o < a.n[i]) adam_element(a, k, a.p[i], a.g[i], a.m[i], a.v[i], o);
    adam_close(a, k);
}

}  // namespace evac
