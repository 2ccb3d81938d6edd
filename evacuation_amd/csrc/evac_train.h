// Device code of libevac, part 6: the TRAINER'S UPDATE -- the other half of RPOAgent.learn() (rpo_agent.py:205-283) for the network
// the policy rollout takes (RPOLinearNetwork, hidden width 64): generalised advantage estimation in one launch (k_gae) and the
// gradient of the RPO / PPO loss of one minibatch with respect to all 13 parameter tensors (k_rpo_*), up to and including what
// loss.backward() leaves in .grad; then the optimiser step, clip_grad_norm_ and Adam (k_adam: one more launch), and the whole
// update's epochs and minibatches from one host call (evac_rpo_update).  No env handle: buffers, sizes and a stream.
//
// evac_rpo_minibatch_grad is at most three launches:
//   k_rpo_adv_stats  (norm_adv only) mean and unbiased std of the minibatch's advantages, one workgroup, fixed-order sums in f64
//   k_rpo_grad       grid (P, 2): workgroup (p, net) walks its share of the minibatch for the actor (net 0) or the critic (net 1)
//                    -- the two losses share nothing but the normalised advantage, so they are separate workgroups.  One wave
//                    per sample, lane k = hidden unit k (policy_eval's forward pass).  W2 lies in LDS ONCE, rows padded to 65
//                    words, so the forward pass (lane k reads row k) and the back-propagation (lane j reads column j) are both
//                    conflict-free; W1 lies transposed the same way.  dW2 accumulates as 64 registers per lane (row k: the outer
//                    product of the lane's pre-activation gradient with the broadcast activations), db1 / db2 / dW3 as one each.
//                    dW1 cannot live in registers (D up to 396): the layer-1 pre-activation gradients go to the workspace
//                    ([net][M][64]) and the finishing launch contracts them with the observations.  The waves of a workgroup are
//                    added in wave order through LDS and the workgroup writes ONE partial to the workspace.
//   k_rpo_finish     ten workgroups sum the P partials per gradient entry in the order p = 0..P-1, write the gradients and leave
//                    the sum of squares of what they wrote in a slot; the others each contract 8 columns of a dW1 over one
//                    segment of the minibatch (16 waves, added in wave order) and leave the tile in the workspace; the last
//                    workgroup of a tile to finish (an INTEGER ticket per tile) adds the tile's segments in segment order,
//                    writes those columns of dW1 and their slot.  The last workgroup of all (another integer ticket) adds the
//                    slots in a fixed tree and writes stats_out.
// Nothing is accumulated with floating-point atomics: every output is a fixed-order sum, the same bits on every run and stream.
// Arithmetic: f32, explicit fmaf chains on the VALU (no MFMA: see DESIGN.md section 8).
#pragma once

#include "evac_common.h"

namespace evac {

constexpr uint32_t kStreamRpo = 0x52504f5au;   // 'RPOZ': the RPO perturbation of the mean (Philox counter word 3)
constexpr int kTrainHidden = 64;
constexpr int kTrainMaxObs = 396;
constexpr int kGradWaves = 8;                   // waves per workgroup of k_rpo_grad
constexpr int kGradBlock = kGradWaves * 64;
constexpr int kGradMaxParts = 128;              // partials per net at most
constexpr int kGradSamplesPerWg = 128;          // ... one per 128 samples below that (16 samples per wave)
constexpr int kRowPad = 65;                     // LDS row stride of the 64-wide matrices (conflict-free by row and by column)
constexpr int kRedCols = 68;                    // dW2 row (64) | db2 | db1 | dW3 row 0 | dW3 row 1
// one workgroup's partial, in floats: dW2 [64][64] | db2 | db1 | dW3[0] | dW3[1] | 16 scalars
constexpr int kPartVec = 64 * 64 + 4 * 64;      // 4352
constexpr int kPartScalars = 16;                // db3[2], dlogstd[2], sum pg, sum v, sum -logratio, sum (ratio - 1 - logratio), clip count
constexpr int kPart = kPartVec + kPartScalars;  // 4368
constexpr int kFinishBlock = 1024;
constexpr int kFinishCombineWgs = (kPart + kFinishBlock - 1) / kFinishBlock;   // 5 per net
constexpr int kW1Tile = 8;                      // dW1 columns per finishing workgroup
constexpr int kMaxW1Tiles = (kTrainMaxObs + kW1Tile - 1) / kW1Tile;   // 50
// workspace: header (adv mean, adv std + 1e-8, the ticket) | slots (10 combining workgroups, then one per dW1 tile) | the 2 x 16
//            summed scalars | one ticket per dW1 tile | G1 [2][M][64] | dW1 segments [2][tiles][S][8][64] | partials [2][P][kPart]
constexpr int kWsHeaderBytes = 64;
constexpr int kWsSlotsBytes = 512;              // 10 + 2 x 50 floats
constexpr int kWsScalarsBytes = 128;
constexpr int kWsTicketsBytes = 512;            // 2 x 50 counters
constexpr int kWsFixedBytes = kWsHeaderBytes + kWsSlotsBytes + kWsScalarsBytes + kWsTicketsBytes;

// Segments the minibatch is cut into for dW1.  A segment's workgroup walks M / (16 S) samples per wave and the last workgroup of
// a tile adds S segments: both are chains of dependent memory latencies, balanced near S = 32.  Wide observations (many tiles)
// take fewer segments -- about 128 workgroups per net in all: with 1000-2000 of them the launch took 2.4-3 times as long at
// D = 124 and 396 (measured) -- and no segment has fewer than 64 samples.
__host__ __device__ inline int rpo_w1_segments(int D, int64_t M) {
    const int nt = (D + kW1Tile - 1) / kW1Tile;
    int64_t s = 128 / nt;
    s = s > 32 ? 32 : s;
    const int64_t most = (M + 63) / 64;
    s = s > most ? most : s;
    return (int)(s < 1 ? 1 : s);
}
__host__ __device__ inline int rpo_parts_upper(int64_t M) {
    const int64_t p = (M + kGradSamplesPerWg - 1) / kGradSamplesPerWg;
    return (int)(p < 1 ? 1 : (p > kGradMaxParts ? kGradMaxParts : p));
}

// LDS of k_rpo_grad, in floats: W2 [64][65] and W1 transposed [D][65] (later the workgroup's reduction buffer [68][65]), rounded
// to 16 bytes; then per wave the observation, the activations and the gradients; then the waves' scalars
__host__ __device__ inline int rpo_grad_region_floats(int D) {
    const int w = (kTrainHidden + D) * kRowPad, r = kRedCols * kRowPad;
    return ((w > r ? w : r) + 3) & ~3;
}

// The optimiser's header (evac_adam_state_t.header; k_adam below).  It lives on the device so that a captured step counts when
// it is replayed.  The k_rpo_* kernels are templates over an optional trailing argument: k_rpo_*<> (RpoArgs alone) are
// evac_rpo_minibatch_grad's kernels; k_rpo_*<const AdamHeader*> are evac_rpo_update's, which return at once, touching nothing,
// when the header's stop flag is set.
struct AdamHeader {                             // 64 bytes (evac_adam_state_t.header)
    int64_t t;                                  // steps taken
    double P1, P2;                              // beta1 ** t, beta2 ** t as running products (read as 1 while t == 0)
    int32_t stop, steps_run, epochs_run;        // evac_rpo_update's early exit and what ran
    uint32_t ticket;                            // the launch's integer ticket: zero between launches
    int32_t pad[6];
};
static_assert(sizeof(AdamHeader) == 64, "evac_adam_state_t.header is 64 bytes");
__device__ __forceinline__ bool rpo_stopped(const AdamHeader* h) { return h->stop != 0; }

struct RpoNet {
    const float *w1, *b1, *w2, *b2, *w3, *b3;
    float *gw1, *gb1, *gw2, *gb2, *gw3, *gb3;
};
struct RpoArgs {
    RpoNet net[2];                              // actor, critic
    const float* logstd;
    float* glogstd;
    const float *obs, *actions, *logprobs, *adv, *ret, *val;   // [B][D], [B][2], [B] ...
    const int64_t* inds;                        // [M]
    const float* noise;                         // [M][2] or NULL
    float* stats;                               // [8]
    char* ws;
    int64_t B;
    float clip, ent, vf, alpha;
    int norm_adv, clip_vloss;
    int D, M, P, chunk, S;                      // P workgroups per net, `chunk` samples each; S segments of dW1
    uint32_t seed_lo, seed_hi, ctr_lo, ctr_hi;
};

__device__ __forceinline__ void wave_sync() {
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
    __builtin_amdgcn_wave_barrier();
}
__device__ __forceinline__ int64_t rpo_index(const RpoArgs& a, int m) {      // (indices outside the batch never leave it)
    const int64_t i = a.inds[m];
    return i < 0 ? 0 : (i >= a.B ? a.B - 1 : i);
}
__device__ __forceinline__ float* ws_header(char* ws) { return (float*)ws; }
__device__ __forceinline__ unsigned* ws_ticket(char* ws) { return (unsigned*)(ws + 8); }
__device__ __forceinline__ float* ws_slots(char* ws) { return (float*)(ws + kWsHeaderBytes); }
__device__ __forceinline__ float* ws_scalars(char* ws) { return (float*)(ws + kWsHeaderBytes + kWsSlotsBytes); }
__device__ __forceinline__ unsigned* ws_tile_tickets(char* ws) { return (unsigned*)(ws + kWsHeaderBytes + kWsSlotsBytes + kWsScalarsBytes); }
__device__ __forceinline__ float* ws_g1(char* ws) { return (float*)(ws + kWsFixedBytes); }
__device__ __forceinline__ float* ws_w1_parts(char* ws, int M) { return ws_g1(ws) + 2 * (size_t)M * kTrainHidden; }
__host__ __device__ inline size_t rpo_w1_parts_floats(int D, int64_t M) {
    return 2 * (size_t)((D + kW1Tile - 1) / kW1Tile) * (size_t)rpo_w1_segments(D, M) * kW1Tile * kTrainHidden;
}
__device__ __forceinline__ float* ws_parts(char* ws, int M, int D) { return ws_w1_parts(ws, M) + rpo_w1_parts_floats(D, M); }

// (k_gae and k_adam, the two kernels here that are not templates, are defined in evac_train_api.hip: this header is seen by
// two translation units)

// Sum of one double per thread over a 1024-thread workgroup: a fixed tree, the total in every thread.
__device__ __forceinline__ double block_sum_1024(double v, double* buf) {
    const int t = (int)threadIdx.x;
    buf[t] = v;
    __syncthreads();
#pragma unroll 1
    for (int s = 512; s > 0; s >>= 1) {
        if (t < s) buf[t] += buf[t + s];
        __syncthreads();
    }
    const double r = buf[0];
    __syncthreads();
    return r;
}

// rpo_agent.py:250-251: mean and torch's default (unbiased) std of b_advantages[mb_inds]; header = (mean, std + 1e-8)
__device__ __forceinline__ void rpo_adv_stats_body(const RpoArgs& a, double* buf) {
    double s = 0.0, q = 0.0;                   // one pass: in f64 the sum of squares of f32 values loses nothing that matters
#pragma unroll 8
    for (int m = (int)threadIdx.x; m < a.M; m += kFinishBlock) {
        const double v = (double)a.adv[rpo_index(a, m)];
        s += v;
        q += v * v;
    }
    const double n = (double)a.M;
    const double mean = block_sum_1024(s, buf) / n;
    double var = (block_sum_1024(q, buf) - n * mean * mean) / (n - 1.0);
    var = var > 0.0 ? var : 0.0;
    if (threadIdx.x == 0) {
        float* h = ws_header(a.ws);
        h[0] = (float)mean;
        h[1] = (float)sqrt(var) + 1e-8f;
    }
}
template <class... Gate>
__global__ __launch_bounds__(kFinishBlock) void k_rpo_adv_stats(RpoArgs a, Gate... gate) {
    __shared__ double buf[kFinishBlock];
    if constexpr (sizeof...(Gate) != 0) {
        if (rpo_stopped(gate...)) return;
    }
    rpo_adv_stats_body(a, buf);
}

template <bool ACTOR>
__device__ __forceinline__ void rpo_grad_body(const RpoArgs& a, float* lds) {
    constexpr int H = kTrainHidden;
    const RpoNet& n = a.net[ACTOR ? 0 : 1];
    const int D = a.D, M = a.M, tid = (int)threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int Dp = (D + 3) & ~3;
    const int region = rpo_grad_region_floats(D);
    float* w2p = lds;                          // [k][j], row stride 65
    float* w1t = lds + H * kRowPad;            // [j][k], row stride 65
    float* rows = lds + region;
    float* xs = rows + wave * (Dp + 2 * H);    // this wave's observation, layer-1 activations, layer-2 pre-activation gradients
    float* h1s = xs + Dp;
    float* g2s = h1s + H;
    float* sc = rows + kGradWaves * (Dp + 2 * H);   // [wave][16]
    for (int i = tid; i < H * H; i += kGradBlock) w2p[(i >> 6) * kRowPad + (i & 63)] = n.w2[i];
    for (int i = tid; i < H * D; i += kGradBlock) {
        const int k = i / D, j = i - k * D;
        w1t[j * kRowPad + k] = n.w1[i];
    }
    __syncthreads();
    const float b1 = n.b1[lane], b2 = n.b2[lane], w30 = n.w3[lane], w31 = ACTOR ? n.w3[H + lane] : 0.0f;
    const float b30 = n.b3[0], b31 = ACTOR ? n.b3[1] : 0.0f;
    constexpr float kLogSqrt2Pi = 0.91893853320467274f;
    float ls0 = 0.0f, ls1 = 0.0f, var0 = 1.0f, var1 = 1.0f;
    if constexpr (ACTOR) {
        ls0 = a.logstd[0];
        ls1 = a.logstd[1];
        const float sd0 = expf(ls0), sd1 = expf(ls1);
        var0 = sd0 * sd0;
        var1 = sd1 * sd1;
    }
    const float inv_m = 1.0f / (float)M;
    const float lo = 1.0f - a.clip, hi = 1.0f + a.clip;
    float adv_mean = 0.0f, adv_den = 1.0f;
    if (ACTOR && a.norm_adv) {
        adv_mean = ws_header(a.ws)[0];
        adv_den = ws_header(a.ws)[1];
    }
    float acc[H];
#pragma unroll
    for (int j = 0; j < H; ++j) acc[j] = 0.0f;
    float gb1 = 0.0f, gb2 = 0.0f, gw30 = 0.0f, gw31 = 0.0f;
    float s_b30 = 0.0f, s_b31 = 0.0f, s_ls0 = 0.0f, s_ls1 = 0.0f, s_loss = 0.0f, s_okl = 0.0f, s_kl = 0.0f, s_clip = 0.0f;
    float* g1_out = ws_g1(a.ws) + (size_t)(ACTOR ? 0 : 1) * (size_t)M * H;
    const int m_begin = (int)blockIdx.x * a.chunk;
    const int m_end = m_begin + a.chunk < M ? m_begin + a.chunk : M;
#pragma unroll 1
    for (int m = m_begin + wave; m < m_end; m += kGradWaves) {
        const int64_t idx = rpo_index(a, m);
        const float* __restrict__ xr = a.obs + (size_t)idx * (size_t)D;
        for (int j = lane; j < D; j += 64) xs[j] = xr[j];
        wave_sync();
        // forward: lane k = hidden unit k
        float p = b1;
#pragma unroll 4
        for (int j = 0; j < D; ++j) p = fmaf(w1t[j * kRowPad + lane], xs[j], p);
        const float h1 = tanhf(p);
        h1s[lane] = h1;
        wave_sync();
        float q = b2;
        const float* w2row = w2p + lane * kRowPad;
#pragma unroll
        for (int g = 0; g < H / 4; ++g) {
            const f4 hv = *(const f4*)(h1s + 4 * g);
            q = fmaf(w2row[4 * g], hv.x, q);
            q = fmaf(w2row[4 * g + 1], hv.y, q);
            q = fmaf(w2row[4 * g + 2], hv.z, q);
            q = fmaf(w2row[4 * g + 3], hv.w, q);
        }
        const float h2 = tanhf(q);
        float o0 = w30 * h2, o1 = w31 * h2, o2 = 0.0f;
        wave_sum3(o0, o1, o2);
        // the loss of this sample and its derivative with respect to the network's outputs (wave-uniform)
        float dh2, gm0 = 0.0f, gm1 = 0.0f;
        if constexpr (ACTOR) {
            float z0, z1;
            if (a.noise) {
                z0 = a.noise[2 * (size_t)m];
                z1 = a.noise[2 * (size_t)m + 1];
            } else {
                const uint4 r = philox4x32_10(make_uint4((uint32_t)m, a.ctr_lo, a.ctr_hi, kStreamRpo), a.seed_lo, a.seed_hi);
                z0 = a.alpha * usym(r.x);
                z1 = a.alpha * usym(r.y);
            }
            const float mean0 = (o0 + b30) + z0, mean1 = (o1 + b31) + z1;      // rpo_linear_agent_network.py:55-59
            const float d0 = a.actions[2 * (size_t)idx] - mean0, d1 = a.actions[2 * (size_t)idx + 1] - mean1;
            const float lp = (-(d0 * d0) / (2.0f * var0) - ls0 - kLogSqrt2Pi) + (-(d1 * d1) / (2.0f * var1) - ls1 - kLogSqrt2Pi);
            const float logratio = lp - a.logprobs[idx];
            const float ratio = expf(logratio);
            float adv = a.adv[idx];
            if (a.norm_adv) adv = (adv - adv_mean) / adv_den;
            const float pg1 = -adv * ratio, pg2 = -adv * fminf(fmaxf(ratio, lo), hi);
            // torch's sub-gradients: clamp passes 1 on the closed interval, max splits a tie half and half
            const float t1 = -adv, t2 = (ratio >= lo && ratio <= hi) ? -adv : 0.0f;
            const float g_ratio = pg1 > pg2 ? t1 : (pg1 < pg2 ? t2 : 0.5f * (t1 + t2));
            const float g_lp = g_ratio * ratio * inv_m;
            gm0 = g_lp * (d0 / var0);
            gm1 = g_lp * (d1 / var1);
            s_ls0 += g_lp * (d0 * d0 / var0 - 1.0f);
            s_ls1 += g_lp * (d1 * d1 / var1 - 1.0f);
            s_b30 += gm0;
            s_b31 += gm1;
            s_loss += fmaxf(pg1, pg2);
            s_okl += -logratio;
            s_kl += (ratio - 1.0f) - logratio;
            s_clip += fabsf(ratio - 1.0f) > a.clip ? 1.0f : 0.0f;
            dh2 = gm0 * w30 + gm1 * w31;
        } else {
            const float v = o0 + b30, R = a.ret[idx];
            const float du = v - R;
            float g_v;
            if (a.clip_vloss) {                                               // rpo_agent.py:260-269
                const float V = a.val[idx], dv = v - V;
                const float dc = (V + fminf(fmaxf(dv, -a.clip), a.clip)) - R;
                const float vu = du * du, vc = dc * dc;
                const float t1 = 2.0f * du, t2 = (dv >= -a.clip && dv <= a.clip) ? 2.0f * dc : 0.0f;
                g_v = 0.5f * (vu > vc ? t1 : (vu < vc ? t2 : 0.5f * (t1 + t2)));
                s_loss += fmaxf(vu, vc);
            } else {                                                          // rpo_agent.py:271
                g_v = du;
                s_loss += du * du;
            }
            gm0 = a.vf * g_v * inv_m;
            s_b30 += gm0;
            dh2 = gm0 * w30;
        }
        // backward
        gw30 = fmaf(gm0, h2, gw30);
        if constexpr (ACTOR) gw31 = fmaf(gm1, h2, gw31);
        const float g2 = dh2 * (1.0f - h2 * h2);
        gb2 += g2;
        g2s[lane] = g2;
#pragma unroll
        for (int g = 0; g < H / 4; ++g) {                                     // dW2[k][.] += g2_k h1[.]
            const f4 hv = *(const f4*)(h1s + 4 * g);
            acc[4 * g] = fmaf(g2, hv.x, acc[4 * g]);
            acc[4 * g + 1] = fmaf(g2, hv.y, acc[4 * g + 1]);
            acc[4 * g + 2] = fmaf(g2, hv.z, acc[4 * g + 2]);
            acc[4 * g + 3] = fmaf(g2, hv.w, acc[4 * g + 3]);
        }
        wave_sync();
        float r = 0.0f;                                                       // lane j: sum_k W2[k][j] g2_k
#pragma unroll
        for (int g = 0; g < H / 4; ++g) {
            const f4 gv = *(const f4*)(g2s + 4 * g);
            r = fmaf(w2p[(4 * g) * kRowPad + lane], gv.x, r);
            r = fmaf(w2p[(4 * g + 1) * kRowPad + lane], gv.y, r);
            r = fmaf(w2p[(4 * g + 2) * kRowPad + lane], gv.z, r);
            r = fmaf(w2p[(4 * g + 3) * kRowPad + lane], gv.w, r);
        }
        const float g1 = r * (1.0f - h1 * h1);
        gb1 += g1;
        g1_out[(size_t)m * H + lane] = g1;
        wave_sync();
    }
    // the workgroup's partial: waves added in wave order through LDS (over the weights, which nobody reads any more)
    if (lane == 0) {
        float* s = sc + wave * kPartScalars;
        s[0] = s_b30; s[1] = s_b31; s[2] = s_ls0; s[3] = s_ls1; s[4] = ACTOR ? s_loss : 0.0f; s[5] = ACTOR ? 0.0f : s_loss;
        s[6] = s_okl; s[7] = s_kl; s[8] = s_clip;
#pragma unroll
        for (int i = 9; i < kPartScalars; ++i) s[i] = 0.0f;
    }
    __syncthreads();
    float* red = lds;                          // [column][lane], row stride 65
#pragma unroll 1
    for (int w = 0; w < kGradWaves; ++w) {
        if (wave == w) {
            if (w == 0) {
#pragma unroll
                for (int j = 0; j < H; ++j) red[j * kRowPad + lane] = acc[j];
                red[64 * kRowPad + lane] = gb2;
                red[65 * kRowPad + lane] = gb1;
                red[66 * kRowPad + lane] = gw30;
                red[67 * kRowPad + lane] = gw31;
            } else {
#pragma unroll
                for (int j = 0; j < H; ++j) red[j * kRowPad + lane] += acc[j];
                red[64 * kRowPad + lane] += gb2;
                red[65 * kRowPad + lane] += gb1;
                red[66 * kRowPad + lane] += gw30;
                red[67 * kRowPad + lane] += gw31;
            }
        }
        __syncthreads();
    }
    float* part = ws_parts(a.ws, M, D) + ((size_t)(ACTOR ? 0 : 1) * a.P + blockIdx.x) * kPart;
    for (int o = tid; o < H * H; o += kGradBlock) part[o] = red[(o & 63) * kRowPad + (o >> 6)];         // dW2[k][j] = column j, lane k
    for (int o = tid; o < 4 * H; o += kGradBlock) part[H * H + o] = red[(64 + (o >> 6)) * kRowPad + (o & 63)];
    if (tid < kPartScalars) {
        float s = 0.0f;
#pragma unroll
        for (int w = 0; w < kGradWaves; ++w) s += sc[w * kPartScalars + tid];
        part[kPartVec + tid] = s;
    }
}

// The first workgroup of the gradient launch clears the tickets of the finishing launch that follows on the stream.
__device__ __forceinline__ void rpo_clear_tickets(char* ws) {
    if (blockIdx.x == 0 && blockIdx.y == 0) {
        if (threadIdx.x == 0) *ws_ticket(ws) = 0u;
        if (threadIdx.x < 2 * kMaxW1Tiles) ws_tile_tickets(ws)[threadIdx.x] = 0u;
    }
}
template <class... Gate>
__global__ __launch_bounds__(kGradBlock) void k_rpo_grad(RpoArgs a, Gate... gate) {
    extern __shared__ __attribute__((aligned(16))) float rpo_lds[];
    if constexpr (sizeof...(Gate) != 0) {
        if (rpo_stopped(gate...)) return;
    }
    rpo_clear_tickets(a.ws);
    if (blockIdx.y == 0) rpo_grad_body<true>(a, rpo_lds);
    else rpo_grad_body<false>(a, rpo_lds);
}

// LDS floats of k_rpo_grad for an observation of D floats
__host__ __device__ inline size_t rpo_grad_lds_floats(int D) {
    const int Dp = (D + 3) & ~3;
    return (size_t)rpo_grad_region_floats(D) + (size_t)kGradWaves * (Dp + 2 * kTrainHidden) + (size_t)kGradWaves * kPartScalars;
}

// Sum of one float per thread over a 1024-thread workgroup: a fixed tree, the total in thread 0's return value.
__device__ __forceinline__ float block_sum_1024f(float v, float* buf) {
    const int t = (int)threadIdx.x;
    buf[t] = v;
    __syncthreads();
#pragma unroll 1
    for (int s = kFinishBlock / 2; s > 0; s >>= 1) {
        if (t < s) buf[t] += buf[t + s];
        __syncthreads();
    }
    const float r = buf[0];
    __syncthreads();
    return r;
}

// The finishing launch's workgroup.  Args = const RpoArgs (BY VALUE) for k_rpo_finish: with a reference the compiler unrolls the
// dW1 loop differently and the kernel no longer compiles to the instructions it had as one function.  The population form
// (evac_population.h) passes a reference to its learner's arguments in LDS: a.net[net] is indexed at run time, which a
// modified private copy could only serve from scratch memory.
template <class Args>
__device__ __forceinline__ void rpo_finish_body(Args a) {
    constexpr int H = kTrainHidden;
    __shared__ float red[16][kW1Tile][H];      // 32 KiB: the 16 waves' dW1 tiles; reused for the sums of squares
    __shared__ float fin[32];
    __shared__ int last;
    const int tid = (int)threadIdx.x, lane = tid & 63, b = (int)blockIdx.x;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int D = a.D, M = a.M, P = a.P, S = a.S;
    const int nt = (D + kW1Tile - 1) / kW1Tile;
    float* w1_parts = ws_w1_parts(a.ws, M);    // [net][tile][segment][column][j]
    if (b < 2 * kFinishCombineWgs) {           // the partials of one net, entry by entry, p = 0..P-1
        const int net = b / kFinishCombineWgs, e = (b % kFinishCombineWgs) * kFinishBlock + tid;
        const RpoNet& n = a.net[net];
        float* dst = nullptr;
        float extra = 0.0f, sq = 0.0f;
        if (e < H * H) dst = n.gw2 + e;
        else if (e < H * H + H) dst = n.gb2 + (e - H * H);
        else if (e < H * H + 2 * H) dst = n.gb1 + (e - H * H - H);
        else if (e < H * H + 3 * H) dst = n.gw3 + (e - H * H - 2 * H);
        else if (e < kPartVec) dst = net == 0 ? n.gw3 + H + (e - H * H - 3 * H) : nullptr;
        else if (e == kPartVec) dst = n.gb3;
        else if (e == kPartVec + 1) dst = net == 0 ? n.gb3 + 1 : nullptr;
        else if (e < kPartVec + 4 && net == 0) {                               // -ent_coef d entropy / d logstd = -ent_coef
            dst = a.glogstd + (e - kPartVec - 2);
            extra = -a.ent;
        }
        if (e < kPart) {
            const float* src = ws_parts(a.ws, M, D) + (size_t)net * P * kPart + e;
            float s = 0.0f;
#pragma unroll 8
            for (int p = 0; p < P; ++p) s += src[(size_t)p * kPart];
            if (e >= kPartVec) ws_scalars(a.ws)[net * kPartScalars + (e - kPartVec)] = s;      // (for the last workgroup)
            if (dst) {
                s += extra;
                *dst = s;
                sq = s * s;
            }
        }
        const float total = block_sum_1024f(sq, &red[0][0][0]);               // the workgroup's sum of squares: a fixed tree
        if (tid == 0) ws_slots(a.ws)[b] = total;
    } else {                                   // segment `seg` of dW1[.][d0 .. d0 + 7] of one net = G1^T X over its samples
        const int bb = b - 2 * kFinishCombineWgs;
        const int seg = bb % S, tile = (bb / S) % nt, net = bb / (S * nt);
        const int d0 = tile * kW1Tile;
        const int nd = D - d0 < kW1Tile ? D - d0 : kW1Tile;
        const float* __restrict__ g1 = ws_g1(a.ws) + (size_t)net * (size_t)M * H;
        const int len = (M + S - 1) / S;
        const int m0 = seg * len, m1 = m0 + len < M ? m0 + len : M;
        float acc[kW1Tile];
#pragma unroll
        for (int c = 0; c < kW1Tile; ++c) acc[c] = 0.0f;
#pragma unroll 8
        for (int m = m0 + wave; m < m1; m += 16) {
            const float g = g1[(size_t)m * H + lane];
            const float* __restrict__ xr = a.obs + (size_t)rpo_index(a, m) * (size_t)D + d0;
#pragma unroll
            for (int c = 0; c < kW1Tile; ++c)
                if (c < nd) acc[c] = fmaf(g, xr[c], acc[c]);
        }
#pragma unroll
        for (int c = 0; c < kW1Tile; ++c) red[wave][c][lane] = acc[c];
        __syncthreads();
        if (tid < kW1Tile * H) {               // the 16 waves in wave order
            const int c = tid >> 6;
            float s = 0.0f;
#pragma unroll
            for (int w = 0; w < 16; ++w) s += red[w][c][lane];
            w1_parts[((size_t)(net * nt + tile) * S + seg) * (kW1Tile * H) + tid] = s;
        }
        // the last workgroup of this tile (an integer ticket) adds the tile's segments in segment order and writes dW1
        __threadfence();
        __syncthreads();
        if (tid == 0) last = atomicAdd(ws_tile_tickets(a.ws) + net * nt + tile, 1u) == (unsigned)S - 1u;
        __syncthreads();
        if (last) {                            // (workgroup-uniform)
            __threadfence();
            float sq = 0.0f;
            if (tid < kW1Tile * H && (tid >> 6) < nd) {
                const float* src = w1_parts + (size_t)(net * nt + tile) * S * (kW1Tile * H) + tid;
                float s = 0.0f;
#pragma unroll 8
                for (int g = 0; g < S; ++g) s += src[(size_t)g * (kW1Tile * H)];
                a.net[net].gw1[(size_t)lane * D + d0 + (tid >> 6)] = s;
                sq = s * s;
            }
            const float total = block_sum_1024f(sq, &red[0][0][0]);
            if (tid == 0) ws_slots(a.ws)[2 * kFinishCombineWgs + net * nt + tile] = total;
        }
        __syncthreads();
    }
    __threadfence();                           // (release: every thread's stores, before the workgroup takes its ticket)
    __syncthreads();
    if (tid == 0) {
        const unsigned ticket = atomicAdd(ws_ticket(a.ws), 1u);
        last = ticket == gridDim.x - 1u;
    }
    __syncthreads();
    if (!last) return;
    __threadfence();
    // the last workgroup to finish: the slots (a fixed tree) and the statistics
    const int n_slots = 2 * kFinishCombineWgs + 2 * nt;
    const float all_sq = block_sum_1024f(tid < n_slots ? ws_slots(a.ws)[tid] : 0.0f, &red[0][0][0]);
    if (tid < kPartScalars) {                  // (the nets' scalars are disjoint: one of the two is zero)
        fin[tid] = ws_scalars(a.ws)[tid] + ws_scalars(a.ws)[kPartScalars + tid];
    } else if (tid == 64) {
        fin[16] = all_sq;
    }
    __syncthreads();
    if (tid == 0) {
        const float inv_m = 1.0f / (float)M;
        const float pg = fin[4] * inv_m, vl = 0.5f * fin[5] * inv_m;
        const float entropy = (0.5f + 0.91893853320467274f + a.logstd[0]) + (0.5f + 0.91893853320467274f + a.logstd[1]);
        a.stats[0] = pg - a.ent * entropy + vl * a.vf;                         // rpo_agent.py:273-274
        a.stats[1] = pg;
        a.stats[2] = vl;
        a.stats[3] = entropy;
        a.stats[4] = fin[6] * inv_m;
        a.stats[5] = fin[7] * inv_m;
        a.stats[6] = fin[8] * inv_m;
        a.stats[7] = fin[16];
    }
}
template <class... Gate>
__global__ __launch_bounds__(kFinishBlock) void k_rpo_finish(RpoArgs a, Gate... gate) {
    if constexpr (sizeof...(Gate) != 0) {
        if (rpo_stopped(gate...)) return;
    }
    rpo_finish_body<const RpoArgs>(a);
}

// ---- rpo_agent.py:278-279: clip_grad_norm_ and Adam(eps = 1e-5).step(), one launch (include/evac.h: evac_adam_step) ----
// A launch of its own behind k_rpo_finish, not a stage of that kernel's last workgroup: the 13 tensors are 9.4 k elements at
// D = 6 and 59 k at D = 396, four arrays each (150 KB .. 950 KB read, all of it written back), which one workgroup
// would walk as a chain of dependent loads of what other workgroups just wrote; a launch spreads them over 37 .. 232 workgroups
// for the price of one kernel boundary, and evac_adam_step (gradients from elsewhere) is then the same kernel, not a twin of it.
// DESIGN.md section 4.6 has the measured cost.
constexpr int kAdamTensors = 13;
constexpr int kAdamBlock = 256;
struct AdamArgs {
    float *p[kAdamTensors], *g[kAdamTensors], *m[kAdamTensors], *v[kAdamTensors];
    int end[kAdamTensors];                      // running element counts: tensor i is [end[i - 1], end[i])
    AdamHeader* hdr;
    const float* sumsq;                         // the sum of squares of all gradient entries (device)
    const float* stats;                         // the step's statistics (approx_kl at [5]) for the early exit, or NULL
    double lr, beta1, beta2, target_kl;
    float max_norm, w, b2, u, eps;              // f32(max_grad_norm), f32(1 - beta1), f32(beta2), f32(1 - beta2), f32(eps)
    int gated, epoch_last, use_target_kl;
};

// Every workgroup forms the scalars from the same inputs (the header is read-only until the last workgroup has its ticket);
// one element per thread; every operation rounded on its own (the sequence of include/evac.h, bit for bit).  sqrt goes through
// double: correctly rounded for a float argument, which the f32 intrinsic of this toolchain is not.
// The three pieces are templates over the argument struct (AdamArgs here; SetAdamArgs of evac_deepsets_adam.h, 19 tensors), which
// names its header, its scalars and its flags alike: k_adam_set shares them, adam_stage is their sequence as it always was.
struct AdamScalars {
    int64_t t0;
    double P1, P2;                              // the header's products after this step
    float c, al, q;                             // the clip coefficient, f32(-(lr / (1 - P1))), f32(sqrt(1 - P2))
};
template <class Args>
__device__ __forceinline__ AdamScalars adam_scalars(const Args& a) {
    const AdamHeader* h = a.hdr;
    AdamScalars k;
    k.t0 = h->t;
    k.P1 = (k.t0 == 0 ? 1.0 : h->P1) * a.beta1;
    k.P2 = (k.t0 == 0 ? 1.0 : h->P2) * a.beta2;
    const float s = *a.sumsq;
    const float x = a.max_norm / __fadd_rn((float)sqrt((double)s), 1e-6f);
    k.c = x > 1.0f ? 1.0f : x;                  // (a NaN stays a NaN, as torch.clamp keeps it)
    k.al = (float)(-(a.lr / (1.0 - k.P1)));
    k.q = (float)sqrt(1.0 - k.P2);
    return k;
}
template <class Args>
__device__ __forceinline__ void adam_element(const Args& a, const AdamScalars& k, float* pp, float* pg, float* pm, float* pv, int o) {
    const float g0 = pg[o], m0 = pm[o], v0 = pv[o], p0 = pp[o];
    const float g = __fmul_rn(g0, k.c);
    const float m = __fadd_rn(m0, __fmul_rn(a.w, __fsub_rn(g, m0)));
    const float v = __fadd_rn(__fmul_rn(v0, a.b2), __fmul_rn(__fmul_rn(a.u, g), g));
    const float den = __fadd_rn((float)sqrt((double)v) / k.q, a.eps);
    pg[o] = g;
    pm[o] = m;
    pv[o] = v;
    pp[o] = __fadd_rn(p0, __fmul_rn(k.al, m) / den);
}
// the last workgroup to finish (an integer ticket) is the one writer of the header: everybody has read it by then
template <class Args>
__device__ __forceinline__ void adam_close(const Args& a, const AdamScalars& k) {
    AdamHeader* h = a.hdr;
    __syncthreads();
    if (threadIdx.x == 0) {
        const unsigned ticket = __hip_atomic_fetch_add(&h->ticket, 1u, __ATOMIC_ACQ_REL, __HIP_MEMORY_SCOPE_AGENT);
        if (ticket == gridDim.x - 1u) {
            h->t = k.t0 + 1;
            h->P1 = k.P1;
            h->P2 = k.P2;
            h->steps_run += 1;
            if (a.epoch_last) {                                               // rpo_agent.py:281-283
                h->epochs_run += 1;
                if (a.use_target_kl && (double)a.stats[5] > a.target_kl) h->stop = 1;
            }
            h->ticket = 0u;
        }
    }
}
__device__ __forceinline__ void adam_stage(const AdamArgs& a) {
    const AdamScalars k = adam_scalars(a);
    const int e = (int)blockIdx.x * kAdamBlock + (int)threadIdx.x;
    if (e < a.end[kAdamTensors - 1]) {
        float *pp = a.p[0], *pg = a.g[0], *pm = a.m[0], *pv = a.v[0];
        int base = 0;
#pragma unroll
        for (int i = 1; i < kAdamTensors; ++i) {
            const bool in = e >= a.end[i - 1];
            pp = in ? a.p[i] : pp;
            pg = in ? a.g[i] : pg;
            pm = in ? a.m[i] : pm;
            pv = in ? a.v[i] : pv;
            base = in ? a.end[i - 1] : base;
        }
        adam_element(a, k, pp, pg, pm, pv, e - base);
    }
    adam_close(a, k);
}
}  // namespace evac
