// Device code of libevac, part 8: the DEEP-SETS LEADER'S GRADIENT -- the RPO minibatch gradient of evac_train.h for the network
// of evac_deepsets.h, all 19 tensors (include/evac.h: evac_deepsets_minibatch_grad).  The actor-critic behind the encoder is
// differentiated by the three kernels of evac_train.h as they are, on the ENCODED observations; three kernels here stand around
// them:
//   k_set_encode     one wave per sample: gathers x = b_obs[inds[m]], runs phases A-C of DeepSetsEncoder::encode (the pooled form,
//                    the same order of sums) and leaves Y[m][D], s[m][24] = W_b t + S b_b and t[m][24] in the workspace, with the
//                    minibatch-ordered copies of actions / logprobs / advantages / returns / values and the index vector 0..M-1:
//                    k_rpo_* then see a batch of M rows whose minibatch is all of it (z and the advantage statistics are keyed
//                    by the position m either way).  Its first workgroup clears the tickets of k_set_finish.
//   k_set_backward   workgroup p walks its share of the minibatch in tiles of 8 samples.  Per tile: dy = W1a^T g1a + W1c^T g1c for
//                    the 8 samples at once (thread = column j; every W1 entry, streamed from L2, serves 8 samples; g1 broadcast
//                    from LDS), stored as dY[m][D]; then one wave per sample: ds = W_r^T dy (24 wave sums over D), dt = W_b^T ds,
//                    the relu masks recomputed from x, and the sample's terms of dW_a, db_a, dW_b, db_b added to per-lane
//                    accumulators (lane = unit x element-residue for dW_a / db_a, lane = column for dW_b).  The waves are added in
//                    wave order through LDS and the workgroup writes ONE partial.
//   k_set_finish     dW_r = dY^T s and db_r = sum_m dY in tiles of 64 columns over segments of the minibatch; the last workgroup
//                    of a tile (an INTEGER ticket) adds the segments in order.  One more workgroup adds the partials of the four
//                    small tensors in workgroup order.  The last workgroup of all adds the slots' sums of squares to stats[7].
// (templates over an optional stop gate: see above k_set_encode.)
// Every sum has a fixed order, no floating-point atomics: the same bits on every run and stream.  f32 fmaf chains on the VALU
// (no MFMA: contractions of M x 24 are far below where it pays).
#pragma once

#include "evac_train.h"

namespace evac {

constexpr int kSetTrainHidden = 24;             // (kSetHidden's: both asserted against evac_host.h's)
constexpr int kSetTrainMaxElemDim = 6;
constexpr int kSetBlock = 256;                  // 4 waves
constexpr int kSetWaves = kSetBlock / 64;
constexpr int kSetTile = 8;                     // samples per dy tile of k_set_backward
constexpr int kSetSamplesPerWg = 32;
constexpr int kSetMaxParts = 512;               // workgroups of k_set_backward at most
constexpr int kSetEncodeMaxWgs = 2048;
constexpr int kSetRowMax = (kTrainMaxObs + 3) & ~3;                       // 396
// one workgroup's partial, in floats: (dW_a[k][0..5], db_a[k]) [24][7] | dW_b [24][24] | db_b [24]
constexpr int kSetPartA = kSetTrainHidden * 7;                            // 168
constexpr int kSetPartB = kSetTrainHidden * kSetTrainHidden;              // 576
constexpr int kSetPart = kSetPartA + kSetPartB + kSetTrainHidden;         // 768
constexpr int kSetWaveRed = 2 * kSetPartA + kSetPartB + kSetTrainHidden;  // 936: a wave's accumulators, both residues
constexpr int kSetRTile = 64;                   // dW_r columns per finishing workgroup
constexpr int kSetMaxRTiles = (kTrainMaxObs + kSetRTile - 1) / kSetRTile; // 7
constexpr int kSetRRows = kSetTrainHidden + 1;  // dW_r[.][0..23] | db_r
constexpr int kSetMaxSegments = 32;
constexpr int kSetHeaderBytes = 128;            // tickets [8] (0: the launch's, 1 + tile: the tiles') | slots [8] (tiles, 7: small)

__host__ __device__ inline int set_parts(int64_t M) {
    const int64_t p = (M + kSetSamplesPerWg - 1) / kSetSamplesPerWg;
    return (int)(p < 1 ? 1 : (p > kSetMaxParts ? kSetMaxParts : p));
}
__host__ __device__ inline int set_segments(int64_t M) {
    const int64_t s = (M + 63) / 64;
    return (int)(s < 1 ? 1 : (s > kSetMaxSegments ? kSetMaxSegments : s));
}

struct SetArgs {
    const float *phi_w1, *phi_b1, *phi_w2, *phi_b2, *rho_w, *rho_b;
    float *g_phi_w1, *g_phi_b1, *g_phi_w2, *g_phi_b2, *g_rho_w, *g_rho_b;
    const float *w1a, *w1c;                     // the actor's and the critic's first layer [64][D]
    const float *obs, *actions, *logprobs, *adv, *ret, *val;   // the caller's batch
    const int64_t* inds;                        // [M]
    int64_t B;
    // the workspace
    float *Y, *dY, *sv, *tv;                    // [M][D], [M][D], [M][24], [M][24]
    float *act_g, *lp_g, *adv_g, *ret_g, *val_g;   // the minibatch in order: [M][2], [M] ...
    int64_t* ident;                             // 0 .. M-1
    const float* g1;                            // [2][M][64]: the layer-1 pre-activation gradients k_rpo_grad left
    float *parts, *rparts;                      // [P][kSetPart], [tiles][Sr][25][64]
    unsigned* tickets;
    float* slots;
    float* stats;
    int D, M, ed, S;                            // S = D / ed rows of ed floats
    int P, chunk;                               // workgroups of k_set_backward, `chunk` samples each
    int Sr, seglen;                             // segments of dW_r, `seglen` samples each
};

__device__ __forceinline__ int64_t set_index(const SetArgs& a, int m) {         // (indices outside the batch never leave it)
    const int64_t i = a.inds[m];
    return i < 0 ? 0 : (i >= a.B ? a.B - 1 : i);
}

// W_a, b_a as two 16-byte vectors per unit: (W_a[k][0..3]), (W_a[k][4], W_a[k][5], b_a[k], -); columns >= ed are 0
__device__ __forceinline__ void set_stage_wa(const SetArgs& a, f4 (*wa)[2]) {
    const int ed = a.ed;
    for (int k = (int)threadIdx.x; k < kSetTrainHidden; k += kSetBlock) {
        float w[kSetTrainMaxElemDim];
#pragma unroll
        for (int c = 0; c < kSetTrainMaxElemDim; ++c) w[c] = c < ed ? a.phi_w1[k * ed + c] : 0.0f;
        wa[k][0] = f4{w[0], w[1], w[2], w[3]};
        wa[k][1] = f4{w[4], w[5], a.phi_b1[k], 0.0f};
    }
}
// the pre-activation of unit k for an element: c ascending from the bias, as DeepSetsEncoder::encode
__device__ __forceinline__ float set_preact(const f4 w0, const f4 w1, const float* x) {
    float v = w1.z;
    v = fmaf(w0.x, x[0], v); v = fmaf(w0.y, x[1], v); v = fmaf(w0.z, x[2], v); v = fmaf(w0.w, x[3], v);
    v = fmaf(w1.x, x[4], v); v = fmaf(w1.y, x[5], v);
    return v;
}

// The POPULATION form (include/evac.h: evac_deepsets_update_population): the learner is blockIdx.y, `a` holds learner 0's
// pointers and the workgroup moves them to its learner's before anything else.  Parameters and gradients by the tensors' strides;
// what lies in a learner's workspace slice (dY, s, t, g1, the partials, tickets and slots) by the slice; what the actor-critic's
// kernels read as ONE common batch of S x M rows -- Y, the gathered columns and the index list -- by the learner's M rows.  The
// caller's batch (obs .. val) is common and stays.  Every shift is a scalar multiply-add on a pointer from the kernel-argument
// segment; gridDim.x is the lone kernel's, so the ticket tests hold per learner.
struct SetLearnerStrides {
    int64_t p[6], g[6];                         // floats from learner s to s + 1: the encoder's parameters, gradients
    int64_t w1a, w1c;                           // ... the actor's and the critic's first layer
    int64_t hdr, ws;                            // bytes: the optimiser's header, the workspace slice
    int64_t inds, stats;                        // elements of perms / stats_out per learner
};
template <class T>
__device__ __forceinline__ T* set_shift_bytes(T* p, int64_t bytes) { return (T*)((char*)p + bytes); }
// Moves `a` to the workgroup's learner; returns the learner's header (the stop gate).
__device__ __forceinline__ const AdamHeader* set_learner(SetArgs& a, const AdamHeader* h, const SetLearnerStrides& q) {
    const int64_t s = (int64_t)blockIdx.y;
    a.phi_w1 += s * q.p[0]; a.phi_b1 += s * q.p[1]; a.phi_w2 += s * q.p[2]; a.phi_b2 += s * q.p[3]; a.rho_w += s * q.p[4]; a.rho_b += s * q.p[5];
    a.g_phi_w1 += s * q.g[0]; a.g_phi_b1 += s * q.g[1]; a.g_phi_w2 += s * q.g[2]; a.g_phi_b2 += s * q.g[3];
    a.g_rho_w += s * q.g[4]; a.g_rho_b += s * q.g[5];
    a.w1a += s * q.w1a; a.w1c += s * q.w1c;
    a.inds += s * q.inds;
    a.stats += s * q.stats;
    const int64_t rows = s * a.M, slice = s * q.ws;
    a.Y += rows * a.D;
    a.act_g += 2 * rows; a.lp_g += rows; a.adv_g += rows; a.ret_g += rows; a.val_g += rows; a.ident += rows;
    a.dY = set_shift_bytes(a.dY, slice); a.sv = set_shift_bytes(a.sv, slice); a.tv = set_shift_bytes(a.tv, slice);
    a.g1 = set_shift_bytes(a.g1, slice); a.parts = set_shift_bytes(a.parts, slice); a.rparts = set_shift_bytes(a.rparts, slice);
    a.tickets = set_shift_bytes(a.tickets, slice); a.slots = set_shift_bytes(a.slots, slice);
    return (const AdamHeader*)((const char*)h + s * q.hdr);
}
// the first index of the workgroup's learner in the common index list (0 for a lone learner)
template <class... Gate>
__device__ __forceinline__ int64_t set_ident_base(int M) {
    if constexpr (sizeof...(Gate) == 2) return (int64_t)blockIdx.y * M;
    else return 0;
}

// The three kernels are templates over an optional trailing argument, as k_rpo_* of evac_train.h: k_set_*<> (SetArgs alone) are
// evac_deepsets_minibatch_grad's and evac_deepsets_minibatch_step's; k_set_*<const AdamHeader*> are evac_deepsets_update's, which
// return at once, touching nothing, when the header's stop flag is set (a gated k_set_encode then leaves k_set_finish's tickets
// as they are: every later kernel of the call returns too); k_set_*<const AdamHeader*, SetLearnerStrides> are the population's
// (above), whose two lines -- the first `if constexpr` and set_ident_base -- the other two forms compile to what they had: the device assembly
// of k_set_*<> and k_set_*<const AdamHeader*> is line for line what it was without them.  The bodies stay
// inside the kernels: moved into __device__
// functions (SetArgs by reference, by value, const or not) all three compiled to other instructions than as plain kernels, and
// k_set_backward began to keep scalars in VGPR lanes; as written, k_set_*<> are instruction for instruction what they were.
template <class... Gate>
__global__ __launch_bounds__(kSetBlock) void k_set_encode(SetArgs a, Gate... gate) {
    if constexpr (sizeof...(Gate) == 2) {
        if (rpo_stopped(set_learner(a, gate...))) return;
    } else if constexpr (sizeof...(Gate) != 0) {
        if (rpo_stopped(gate...)) return;
    }
    constexpr int H = kSetTrainHidden;
    __shared__ f4 wa[H][2];
    __shared__ float wb[H][H];                  // [j][k] = W_b[k][j]
    __shared__ float bb[H];
    __shared__ __attribute__((aligned(16))) float xs_all[kSetWaves][kSetRowMax];
    __shared__ __attribute__((aligned(16))) float ts_all[kSetWaves][2 * H];
    const int tid = (int)threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int D = a.D, M = a.M, ed = a.ed, S = a.S;
    if (blockIdx.x == 0 && tid < 16) a.tickets[tid] = 0u;      // (k_set_finish's tickets; the slots behind them are written there)
    set_stage_wa(a, wa);
    for (int idx = tid; idx < H * H; idx += kSetBlock) {
        const int j = idx / H, k = idx % H;
        wb[j][k] = a.phi_w2[k * H + j];
    }
    if (tid < H) bb[tid] = a.phi_b2[tid];
    __syncthreads();
    float* xs = xs_all[wave];
    float* t = ts_all[wave];
#pragma unroll 1
    for (int m = (int)blockIdx.x * kSetWaves + wave; m < M; m += (int)gridDim.x * kSetWaves) {
        const int64_t idx = set_index(a, m);
        const float* __restrict__ xr = a.obs + (size_t)idx * (size_t)D;
        for (int j = lane; j < D; j += 64) xs[j] = xr[j];
        if (lane < 2) a.act_g[2 * (size_t)m + lane] = a.actions[2 * (size_t)idx + lane];
        else if (lane == 2) a.lp_g[m] = a.logprobs[idx];
        else if (lane == 3) a.adv_g[m] = a.adv[idx];
        else if (lane == 4) a.ret_g[m] = a.ret[idx];
        else if (lane == 5) a.val_g[m] = a.val[idx];
        else if (lane == 6) a.ident[m] = set_ident_base<Gate...>(M) + (int64_t)m;
        wave_sync();
        // A: the pooled hidden sums
        for (int base = 0; base < S; base += 64) {
            const int i = base + lane;
            const bool valid = i < S;
            float x[kSetTrainMaxElemDim];
#pragma unroll
            for (int c = 0; c < kSetTrainMaxElemDim; ++c) x[c] = (valid && c < ed) ? xs[i * ed + c] : 0.0f;
#pragma unroll 1
            for (int k = 0; k < H; k += 3) {
                float h[3];
#pragma unroll
                for (int u = 0; u < 3; ++u) {
                    float v = set_preact(wa[k + u][0], wa[k + u][1], x);
                    v = v < 0.0f ? 0.0f : v;           // relu (a NaN stays one)
                    h[u] = valid ? v : 0.0f;
                }
                wave_sum3(h[0], h[1], h[2]);
                if (lane < 3) {
                    float v = lane == 0 ? h[0] : (lane == 1 ? h[1] : h[2]);
                    if (base != 0) v = t[k + lane] + v;
                    t[k + lane] = v;
                }
            }
        }
        wave_sync();
        // B: s = W_b t + S b_b
        if (lane < H) {
            float s = (float)S * bb[lane];
#pragma unroll
            for (int j = 0; j < H; ++j) s = fmaf(wb[j][lane], t[j], s);
            t[H + lane] = s;
            a.tv[(size_t)m * H + lane] = t[lane];
            a.sv[(size_t)m * H + lane] = s;
        }
        wave_sync();
        // C: y = W_r s + b_r
        const f4* sv4 = (const f4*)(t + H);
        float* __restrict__ yr = a.Y + (size_t)m * (size_t)D;
#pragma unroll 1
        for (int j = lane; j < D; j += 64) {
            const f4* __restrict__ r = (const f4*)(a.rho_w + (size_t)j * H);
            float v = a.rho_b[j];
#pragma unroll
            for (int g = 0; g < H / 4; ++g) {
                const f4 w = r[g], s = sv4[g];
                v = fmaf(w.x, s.x, v); v = fmaf(w.y, s.y, v); v = fmaf(w.z, s.z, v); v = fmaf(w.w, s.w, v);
            }
            yr[j] = v;
        }
        wave_sync();
    }
}

template <class... Gate>
__global__ __launch_bounds__(kSetBlock) void k_set_backward(SetArgs a, Gate... gate) {
    if constexpr (sizeof...(Gate) == 2) {
        if (rpo_stopped(set_learner(a, gate...))) return;
    } else if constexpr (sizeof...(Gate) != 0) {
        if (rpo_stopped(gate...)) return;
    }
    constexpr int H = kSetTrainHidden, H1 = kTrainHidden;
    __shared__ f4 wa[H][2];
    __shared__ float wb[H][H];                  // [k][j] = W_b[k][j]
    __shared__ __attribute__((aligned(16))) float gs[2 * H1][kSetTile];        // g1 of the tile's samples: [net, unit][sample]
    __shared__ __attribute__((aligned(16))) float dys[kSetTile][kSetRowMax];
    __shared__ __attribute__((aligned(16))) float xs_all[kSetWaves][kSetRowMax];
    __shared__ float dss[kSetWaves][H], dts[kSetWaves][H];
    __shared__ float red[kSetWaves][kSetWaveRed];
    const int tid = (int)threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int D = a.D, M = a.M, ed = a.ed, S = a.S;
    set_stage_wa(a, wa);
    for (int idx = tid; idx < H * H; idx += kSetBlock) wb[idx / H][idx % H] = a.phi_w2[idx];
    __syncthreads();
    const int ku = lane % H, res = lane / H;    // lanes < 48: unit ku, elements res, res + 2, ...
    const f4 wk0 = wa[ku][0], wk1 = wa[ku][1];
    float gwa[kSetTrainMaxElemDim], gba = 0.0f, gbb = 0.0f;
    float gwb[H];                               // lane j < 24: dW_b[.][j]
#pragma unroll
    for (int c = 0; c < kSetTrainMaxElemDim; ++c) gwa[c] = 0.0f;
#pragma unroll
    for (int k = 0; k < H; ++k) gwb[k] = 0.0f;
    const float Sf = (float)S;
    float* xs = xs_all[wave];
    const int m_begin = (int)blockIdx.x * a.chunk;
    const int m_end = m_begin + a.chunk < M ? m_begin + a.chunk : M;
#pragma unroll 1
    for (int m0 = m_begin; m0 < m_end; m0 += kSetTile) {
        const int nq = m_end - m0 < kSetTile ? m_end - m0 : kSetTile;
        // g1 of both nets for the tile's samples (zero beyond the tile's end)
        for (int i = tid; i < 2 * H1 * kSetTile; i += kSetBlock) {
            const int q = i / (2 * H1), r = i - q * (2 * H1);
            const int net = r / H1, k = r - net * H1;
            gs[r][q] = q < nq ? a.g1[((size_t)net * (size_t)M + (size_t)(m0 + q)) * H1 + k] : 0.0f;
        }
        __syncthreads();
        // dy[q][j] = sum_k W1a[k][j] g1a[q][k] + sum_k W1c[k][j] g1c[q][k], k ascending, the actor first
#pragma unroll 1
        for (int j = tid; j < D; j += kSetBlock) {
            float acc[kSetTile];
#pragma unroll
            for (int q = 0; q < kSetTile; ++q) acc[q] = 0.0f;
#pragma unroll 1
            for (int net = 0; net < 2; ++net) {
                const float* __restrict__ w1 = (net == 0 ? a.w1a : a.w1c) + j;
#pragma unroll 8
                for (int k = 0; k < H1; ++k) {
                    const float w = w1[(size_t)k * (size_t)D];
                    const f4 g0 = *(const f4*)&gs[net * H1 + k][0], g1 = *(const f4*)&gs[net * H1 + k][4];
                    acc[0] = fmaf(w, g0.x, acc[0]); acc[1] = fmaf(w, g0.y, acc[1]); acc[2] = fmaf(w, g0.z, acc[2]); acc[3] = fmaf(w, g0.w, acc[3]);
                    acc[4] = fmaf(w, g1.x, acc[4]); acc[5] = fmaf(w, g1.y, acc[5]); acc[6] = fmaf(w, g1.z, acc[6]); acc[7] = fmaf(w, g1.w, acc[7]);
                }
            }
#pragma unroll
            for (int q = 0; q < kSetTile; ++q) {
                dys[q][j] = acc[q];
                if (q < nq) a.dY[(size_t)(m0 + q) * (size_t)D + j] = acc[q];
            }
        }
        __syncthreads();
        // one wave per sample: through the encoder, backwards
#pragma unroll 1
        for (int q = wave; q < nq; q += kSetWaves) {
            const int m = m0 + q;
            const float* __restrict__ xr = a.obs + (size_t)set_index(a, m) * (size_t)D;
            for (int j = lane; j < D; j += 64) xs[j] = xr[j];
            // ds_k = sum_j W_r[j][k] dy_j: the lane's columns j ascending, then the lanes in wave_sum3's tree
            float p[H];
#pragma unroll
            for (int k = 0; k < H; ++k) p[k] = 0.0f;
#pragma unroll 1
            for (int j = lane; j < D; j += 64) {
                const f4* __restrict__ r = (const f4*)(a.rho_w + (size_t)j * H);
                const float dy = dys[q][j];
#pragma unroll
                for (int g = 0; g < H / 4; ++g) {
                    const f4 w = r[g];
                    p[4 * g] = fmaf(w.x, dy, p[4 * g]); p[4 * g + 1] = fmaf(w.y, dy, p[4 * g + 1]);
                    p[4 * g + 2] = fmaf(w.z, dy, p[4 * g + 2]); p[4 * g + 3] = fmaf(w.w, dy, p[4 * g + 3]);
                }
            }
#pragma unroll
            for (int k = 0; k < H; k += 3) wave_sum3(p[k], p[k + 1], p[k + 2]);               // (the totals in every lane)
            if (lane == 0) {
#pragma unroll
                for (int k = 0; k < H; ++k) dss[wave][k] = p[k];
            }
            wave_sync();
            if (lane < H) {
                const float tj = a.tv[(size_t)m * H + lane];
                gbb = fmaf(Sf, dss[wave][lane], gbb);                                          // db_b += S ds
                float dt = 0.0f;
#pragma unroll
                for (int k = 0; k < H; ++k) {
                    gwb[k] = fmaf(p[k], tj, gwb[k]);                                           // dW_b[k][j] += ds_k t_j
                    dt = fmaf(wb[k][lane], p[k], dt);                                          // dt_j = sum_k W_b[k][j] ds_k
                }
                dts[wave][lane] = dt;
            }
            wave_sync();
            if (lane < 2 * H) {                                                               // dh_ik = dt_k [a_ik > 0]
                const float dtk = dts[wave][ku];
#pragma unroll 1
                for (int i = res; i < S; i += 2) {
                    float x[kSetTrainMaxElemDim];
#pragma unroll
                    for (int c = 0; c < kSetTrainMaxElemDim; ++c) x[c] = c < ed ? xs[i * ed + c] : 0.0f;
                    const float dh = set_preact(wk0, wk1, x) > 0.0f ? dtk : 0.0f;
                    gba += dh;
#pragma unroll
                    for (int c = 0; c < kSetTrainMaxElemDim; ++c) gwa[c] = fmaf(dh, x[c], gwa[c]);
                }
            }
            wave_sync();
        }
        __syncthreads();
    }
    // the workgroup's partial: per entry the waves in wave order, a wave's two residues in order
    float* mine = red[wave];
    if (lane < 2 * H) {
#pragma unroll
        for (int c = 0; c < kSetTrainMaxElemDim; ++c) mine[res * kSetPartA + ku * 7 + c] = gwa[c];
        mine[res * kSetPartA + ku * 7 + 6] = gba;
    }
    if (lane < H) {
#pragma unroll
        for (int k = 0; k < H; ++k) mine[2 * kSetPartA + k * H + lane] = gwb[k];
        mine[2 * kSetPartA + kSetPartB + lane] = gbb;
    }
    __syncthreads();
    float* part = a.parts + (size_t)blockIdx.x * kSetPart;
    for (int e = tid; e < kSetPart; e += kSetBlock) {
        float s = 0.0f;
        if (e < kSetPartA) {
#pragma unroll
            for (int w = 0; w < kSetWaves; ++w) {
                s += red[w][e];
                s += red[w][kSetPartA + e];
            }
        } else {
#pragma unroll
            for (int w = 0; w < kSetWaves; ++w) s += red[w][kSetPartA + e];
        }
        part[e] = s;
    }
}

// Sum of one float per thread over the workgroup: a fixed tree, the total in thread 0's return value.
__device__ __forceinline__ float set_block_sum(float v, float* buf) {
    const int t = (int)threadIdx.x;
    buf[t] = v;
    __syncthreads();
#pragma unroll 1
    for (int s = kSetBlock / 2; s > 0; s >>= 1) {
        if (t < s) buf[t] += buf[t + s];
        __syncthreads();
    }
    const float r = buf[0];
    __syncthreads();
    return r;
}

template <class... Gate>
__global__ __launch_bounds__(kSetBlock) void k_set_finish(SetArgs a, Gate... gate) {
    if constexpr (sizeof...(Gate) == 2) {
        if (rpo_stopped(set_learner(a, gate...))) return;
    } else if constexpr (sizeof...(Gate) != 0) {
        if (rpo_stopped(gate...)) return;
    }
    constexpr int H = kSetTrainHidden;
    __shared__ float buf[kSetBlock];
    __shared__ float fin[8];
    __shared__ int last;
    const int tid = (int)threadIdx.x, lane = tid & 63, b = (int)blockIdx.x;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int D = a.D, M = a.M, Sr = a.Sr;
    const int nt = (D + kSetRTile - 1) / kSetRTile;
    if (b < nt * Sr) {                         // segment `seg` of dW_r[j0 .. j0 + 63][.] and db_r: wave w owns units 6 w .. 6 w + 5
        const int tile = b / Sr, seg = b - tile * Sr;
        const int j = tile * kSetRTile + lane;
        const bool valid = j < D;
        const int m0 = seg * a.seglen, m1 = m0 + a.seglen < M ? m0 + a.seglen : M;
        const int k0 = wave * 6;
        float acc[6], accb = 0.0f;
#pragma unroll
        for (int c = 0; c < 6; ++c) acc[c] = 0.0f;
#pragma unroll 4
        for (int m = m0; m < m1; ++m) {
            const float dy = valid ? a.dY[(size_t)m * (size_t)D + j] : 0.0f;
            const float* __restrict__ s = a.sv + (size_t)m * H + k0;
#pragma unroll
            for (int c = 0; c < 6; ++c) acc[c] = fmaf(dy, s[c], acc[c]);
            accb += dy;
        }
        float* seg_out = a.rparts + (size_t)(tile * Sr + seg) * (kSetRRows * kSetRTile);
#pragma unroll
        for (int c = 0; c < 6; ++c) seg_out[(k0 + c) * kSetRTile + lane] = acc[c];
        if (wave == 0) seg_out[H * kSetRTile + lane] = accb;
        // the last workgroup of this tile (an integer ticket) adds the tile's segments in segment order
        __threadfence();
        __syncthreads();
        if (tid == 0) last = atomicAdd(a.tickets + 1 + tile, 1u) == (unsigned)Sr - 1u;
        __syncthreads();
        if (last) {                            // (workgroup-uniform)
            __threadfence();
            float sq = 0.0f;
            const float* src = a.rparts + (size_t)tile * Sr * (kSetRRows * kSetRTile) + lane;
#pragma unroll 1
            for (int c = 0; c < 7; ++c) {
                if (c == 6 && wave != 0) break;
                const int row = c < 6 ? k0 + c : H;
                float s = 0.0f;
#pragma unroll 8
                for (int g = 0; g < Sr; ++g) s += src[((size_t)g * kSetRRows + row) * kSetRTile];
                if (valid) {
                    if (c < 6) a.g_rho_w[(size_t)j * H + row] = s;
                    else a.g_rho_b[j] = s;
                    sq = fmaf(s, s, sq);
                }
            }
            const float total = set_block_sum(sq, buf);
            if (tid == 0) a.slots[tile] = total;
        }
    } else {                                   // the four small tensors: the partials of k_set_backward in workgroup order
        const int ed = a.ed, P = a.P;
        float sq = 0.0f;
        for (int e = tid; e < kSetPart; e += kSetBlock) {
            const float* src = a.parts + e;
            float s = 0.0f;
#pragma unroll 8
            for (int p = 0; p < P; ++p) s += src[(size_t)p * kSetPart];
            float* dst = nullptr;
            if (e < kSetPartA) {
                const int k = e / 7, c = e - k * 7;
                if (c == 6) dst = a.g_phi_b1 + k;
                else if (c < ed) dst = a.g_phi_w1 + k * ed + c;
            } else if (e < kSetPartA + kSetPartB) {
                dst = a.g_phi_w2 + (e - kSetPartA);
            } else {
                dst = a.g_phi_b2 + (e - kSetPartA - kSetPartB);
            }
            if (dst) {
                *dst = s;
                sq = fmaf(s, s, sq);
            }
        }
        const float total = set_block_sum(sq, buf);
        if (tid == 0) a.slots[kSetMaxRTiles] = total;
    }
    __threadfence();                           // (release: every thread's stores, before the workgroup takes its ticket)
    __syncthreads();
    if (tid == 0) last = atomicAdd(a.tickets, 1u) == gridDim.x - 1u;
    __syncthreads();
    if (!last) return;
    __threadfence();
    // the last workgroup to finish: the encoder's sum of squares joins the 13 tensors' (k_rpo_finish wrote stats[7] before this launch)
    if (tid < 8) fin[tid] = tid < nt || tid == kSetMaxRTiles ? a.slots[tid] : 0.0f;
    __syncthreads();
    if (tid == 0) {
        float s = 0.0f;
#pragma unroll
        for (int i = 0; i < 8; ++i) s += fin[i];
        a.stats[7] = a.stats[7] + s;
    }
}

}  // namespace evac
