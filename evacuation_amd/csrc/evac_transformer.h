// Device code of libevac, part 8: the TRANSFORMER LEADER -- the reference's attention encoder (rpo_transformer_agent_network.py)
// in front of the actor-critic of the policy rollout and the policy evaluation.  The Box observation is S = N + 2 tokens
// (leader, exit, pedestrians) of dm = D / S floats; num_blocks blocks map [S][dm] -> [S][dm], each
//     Q, K, V = x W^T + b                                     [S][3 dm], output index h dm + c (3 heads)
//     score[c][i][j] = sum_h Q[i][h dm + c] K[j][h dm + c] / sqrt(dm)     per CHANNEL c, contracted over the heads (the
//     w = softmax_j(score),  o[i][c][h] = sum_j w[c][i][j] V[j][h dm + c]   reference's split_heads permutes to [dm][S][heads])
//     a_i = dense(o[i] flattened as c 3 + h),   u = LayerNorm1(x + a | a),   f = W2 relu(W1 u + b1) + b2,   LayerNorm2(u + f | f)
// (dropout the identity: the eval-mode function) and actor_mean / critic then read the last block's output where
// RPOLinearNetwork reads x.  Everything below the encoder is evac_policy.h / evac_evaluate.h, called through their ENC hook,
// as evac_deepsets.h does.
//
// One wave per env, lane = token, one pass (S <= 64: N <= 62; the host refuses more).  The token's row x[6] goes from block to
// block in registers, columns >= dm zero (every staged weight is zero-padded to 6 columns, so one code path serves dm = 6, 3, 2).
// Per block:
//   attention, one channel c at a time: the lane computes its token's q[3] (W_q, b_q staged times log2(e) / sqrt(dm), so the softmax
//       is exp2) and k[3], v[3], and writes k, v into the wave's OBSERVATION row x as [j][k0 k1 k2 v0 v1 v2] -- that row is dead from
//       the moment every lane has read its token until the body stages the next observation (policy_eval reads row(), not x).
//       Pass 1 over j < S takes the row maximum of the scores, pass 2 sums exp2(score - max) and the three weighted v's, both
//       reading token j's values as LDS broadcasts, j ascending.  o / sum is folded at once into the 6 outputs of `dense`.
//       Lanes >= S compute on zeros and are never read: j stops at S.
//   LayerNorm over the dm values (biased variance, eps = 1e-5, affine), then the feed-forward network streamed unit by unit
//       (96 x 4 broadcast vectors) into 6 accumulators, then the second LayerNorm.
// The last block's output goes to the wave's row of `y`, which row(slot) returns; until then the lane keeps its block's input
// there, so that it is not live through the loops over j.  The weights of both blocks are staged ONCE per workgroup (8 640 B a
// block).  Every sum has a fixed order and no atomics: the result depends on the env's observation and the weights alone.
#pragma once

#include "evac_evaluate.h"

namespace evac {

constexpr int kTfHeads = 3;                      // RPOTransformerEmbeddingConfig.num_heads (the only count the kernels take)
constexpr int kTfFeedForward = 96;               // ... .dim_feedforward (likewise)
constexpr int kTfMaxModelDim = 6;                // positions + one-hot status
constexpr int kTfMaxBlocks = 2;                  // ... .num_blocks: 1 or 2
constexpr float kTfLnEps = 1e-5f;                // nn.LayerNorm's default

// evac_transformer_block_t's tensors (torch layouts, read once per workgroup)
struct TransformerBlockArgs {
    const float *wq, *bq, *wk, *bk, *wv, *bv, *dense_w, *dense_b, *ff1_w, *ff1_b, *ff2_w, *ff2_b, *norm1_w, *norm1_b, *norm2_w, *norm2_b;
};
struct TransformerArgs {
    TransformerBlockArgs blk[kTfMaxBlocks];
    int elem_dim, num_blocks, use_resid;
};

struct TransformerBlockSmem {
    f4 qkv[kTfMaxModelDim][3][kTfHeads][2];      // [c][q | k | v][h]: (W[h dm + c][0..3]), (W[..][4], W[..][5], b[h dm + c], 0); q's times log2(e) / sqrt(dm)
    f4 dn[kTfMaxModelDim][kTfHeads][2];          // [c][h]: (dense_w[0..3][c 3 + h]), (dense_w[4][..], dense_w[5][..], 0, 0)
    f4 ff[kTfFeedForward][4];                    // [u]: (W1[u][0..3]), (W1[u][4], W1[u][5], b1[u], 0), (W2[0..3][u]), (W2[4][u], W2[5][u], 0, 0)
    f4 vec[6][2];                                // dense_b, norm1_w, norm1_b, ff2_b, norm2_w, norm2_b (6 values each, 0-padded)
};

struct TransformerSmem {
    alignas(16) float y[PolicyFamily::kEnvsPerBlock][kPolicyMaxObs];      // the encoded observation the actor-critic reads
    TransformerBlockSmem blk[kTfMaxBlocks];
    int elem_dim, num_blocks, use_resid;                                   // (read back where used, as PolicySmem::args)
};

static_assert(kTfMaxModelDim * kWave <= kPolicyMaxObs, "TransformerEncoder: k, v of 64 tokens in the observation's LDS row");

// a tensor's place in TransformerBlockArgs
enum TransformerTensor {
    kTf_wq, kTf_bq, kTf_wk, kTf_bk, kTf_wv, kTf_bv, kTf_dense_w, kTf_dense_b, kTf_ff1_w, kTf_ff1_b, kTf_ff2_w, kTf_ff2_b,
    kTf_norm1_w, kTf_norm1_b, kTf_norm2_w, kTf_norm2_b, kTfBlockTensors
};
static_assert(sizeof(TransformerBlockArgs) == kTfBlockTensors * sizeof(const float*), "TransformerTensor names every tensor of a block");

// Whose tensors stage() reads: of(tensor i of block b as the launch passed it) is the one to read.  A lone network: that one.
// (A population's learner: evac_transformer_population.h.)
struct TransformerOwnTensors {
    __device__ __forceinline__ const float* of(const float* tensor, int, int) const { return tensor; }
    static constexpr bool kFresh = false;
    static __device__ __forceinline__ int fresh(int v) { return v; }            // (encode()'s lane and row: as they are)
    static __device__ __forceinline__ float* fresh(float* v) { return v; }
};

template <class Tensors>
struct TransformerEncoderOf {
    static constexpr bool kOn = true;
    TransformerSmem& ts;
    const TransformerArgs& ka;
    Tensors whose{};

    // by the whole workgroup, before the staging barrier (beside stage_policy)
    __device__ __forceinline__ void stage() const {
        const int dm = ka.elem_dim, tid = (int)threadIdx.x;
        constexpr int kStep = PolicyFamily::kBlock;
        const float qscale = 1.44269504088896341f / sqrtf((float)dm);   // softmax_j(s / sqrt(dm)) as exp2: log2(e) / sqrt(dm) into W_q, b_q
        for (int b = 0; b < ka.num_blocks; ++b) {
            const TransformerBlockArgs& B = ka.blk[b];
            const auto T = [&](const float* tensor, int i) { return whose.of(tensor, b, i); };
            TransformerBlockSmem& t = ts.blk[b];
            float* qkv = (float*)t.qkv;
            for (int idx = tid; idx < kTfMaxModelDim * 3 * kTfHeads * 8; idx += kStep) {
                const int e = idx & 7, r = idx >> 3, h = r % kTfHeads, m = (r / kTfHeads) % 3, c = r / (3 * kTfHeads);
                const float* W = m == 0 ? T(B.wq, kTf_wq) : (m == 1 ? T(B.wk, kTf_wk) : T(B.wv, kTf_wv));
                const float* bias = m == 0 ? T(B.bq, kTf_bq) : (m == 1 ? T(B.bk, kTf_bk) : T(B.bv, kTf_bv));
                float v = 0.0f;
                if (c < dm) {
                    const int row = h * dm + c;
                    if (e < dm) v = W[row * dm + e];
                    else if (e == 6) v = bias[row];
                    if (m == 0) v *= qscale;
                }
                qkv[idx] = v;
            }
            float* dn = (float*)t.dn;
            for (int idx = tid; idx < kTfMaxModelDim * kTfHeads * 8; idx += kStep) {
                const int e = idx & 7, r = idx >> 3, h = r % kTfHeads, c = r / kTfHeads;
                dn[idx] = (c < dm && e < dm) ? T(B.dense_w, kTf_dense_w)[e * (kTfHeads * dm) + c * kTfHeads + h] : 0.0f;
            }
            float* ff = (float*)t.ff;
            for (int idx = tid; idx < kTfFeedForward * 16; idx += kStep) {
                const int e = idx & 15, u = idx >> 4;
                float v = 0.0f;
                if (e < 8) {
                    if (e < dm) v = T(B.ff1_w, kTf_ff1_w)[u * dm + e];
                    else if (e == 6) v = T(B.ff1_b, kTf_ff1_b)[u];
                } else if (e - 8 < dm) {
                    v = T(B.ff2_w, kTf_ff2_w)[(e - 8) * kTfFeedForward + u];
                }
                ff[idx] = v;
            }
            float* vec = (float*)t.vec;
            for (int idx = tid; idx < 6 * 8; idx += kStep) {
                const int e = idx & 7, r = idx >> 3;
                const float* src = r == 0 ? T(B.dense_b, kTf_dense_b)
                                 : r == 1 ? T(B.norm1_w, kTf_norm1_w)
                                 : r == 2 ? T(B.norm1_b, kTf_norm1_b)
                                 : r == 3 ? T(B.ff2_b, kTf_ff2_b)
                                 : r == 4 ? T(B.norm2_w, kTf_norm2_w)
                                          : T(B.norm2_b, kTf_norm2_b);
                vec[idx] = e < dm ? src[e] : 0.0f;
            }
        }
        if (threadIdx.x == 0) {
            ts.elem_dim = ka.elem_dim;
            ts.num_blocks = ka.num_blocks;
            ts.use_resid = ka.use_resid;
        }
    }

    __device__ __forceinline__ const float* row(int slot) const { return ts.y[slot]; }

    // b + sum_c w[c] x[c] of a staged row (two vectors: six weights, the bias, a zero), c ascending
    static __device__ __forceinline__ float affine6(const f4 w0, const f4 w1, const float (&x)[kTfMaxModelDim]) {
        float v = w1.z;
        v = fmaf(w0.x, x[0], v); v = fmaf(w0.y, x[1], v); v = fmaf(w0.z, x[2], v); v = fmaf(w0.w, x[3], v);
        v = fmaf(w1.x, x[4], v); v = fmaf(w1.y, x[5], v);
        return v;
    }

    // LayerNorm of the dm leading values of v (the others stay 0: their weight and bias are staged as 0)
    static __device__ __forceinline__ void layer_norm(float (&v)[kTfMaxModelDim], int dm, const f4 w0, const f4 w1, const f4 b0, const f4 b1) {
        const float inv = 1.0f / (float)dm;
        const float mean = (((((v[0] + v[1]) + v[2]) + v[3]) + v[4]) + v[5]) * inv;      // (the padding adds zeros)
        float d[kTfMaxModelDim], var = 0.0f;
#pragma unroll
        for (int c = 0; c < kTfMaxModelDim; ++c) {
            d[c] = c < dm ? v[c] - mean : 0.0f;
            var = fmaf(d[c], d[c], var);
        }
        const float rstd = 1.0f / sqrtf(var * inv + kTfLnEps);
        const float w[kTfMaxModelDim] = {w0.x, w0.y, w0.z, w0.w, w1.x, w1.y}, b[kTfMaxModelDim] = {b0.x, b0.y, b0.z, b0.w, b1.x, b1.y};
#pragma unroll
        for (int c = 0; c < kTfMaxModelDim; ++c) v[c] = fmaf(d[c] * rstd, w[c], b[c]);
    }

    // x (the wave's LDS row of D = S x dm floats) -> y (ts.y[slot]); the caller has synchronised x, y is synchronised on return.
    // The row x is overwritten (k, v of the channel at hand).
    __device__ __forceinline__ void encode(float* xs, int slot, int lane, int D, int S) const {
        using F = PolicyFamily;
        // (Tensors::fresh: the value again.  A population's learner makes it opaque, so that the addresses formed from the lane and
        // the row are formed anew at every call and for every channel, not carried in registers through the step loop.)
        lane = Tensors::fresh(lane);
        xs = Tensors::fresh(xs);
        const int dm = ts.elem_dim, nb = ts.num_blocks;
        const bool resid = ts.use_resid != 0;
        const bool valid = lane < S;
        float x[kTfMaxModelDim];
#pragma unroll
        for (int c = 0; c < kTfMaxModelDim; ++c) x[c] = (valid && c < dm) ? xs[lane * dm + c] : 0.0f;
        F::sync();                                                  // every token is in registers: the row is free
        f2* kv = (f2*)xs + 3 * lane;                                // [j][k0 k1 | k2 v0 | v1 v2]
        // The block's input waits in the lane's six floats of the y row while the loops over j run (the step's state leaves no
        // registers for it: the rollout kernels are at the limit of 128), and comes back for each channel's q, k, v.
        f2* keep = (f2*)ts.y[slot] + 3 * lane;
#pragma unroll 1
        for (int b = 0; b < nb; ++b) {
            const TransformerBlockSmem& t = ts.blk[b];
            keep[0] = f2{x[0], x[1]};
            keep[1] = f2{x[2], x[3]};
            keep[2] = f2{x[4], x[5]};
            float a[kTfMaxModelDim] = {t.vec[0][0].x, t.vec[0][0].y, t.vec[0][0].z, t.vec[0][0].w, t.vec[0][1].x, t.vec[0][1].y};
#pragma unroll 1
            for (int c = 0; c < dm; ++c) {
                float q[kTfHeads], kk[kTfHeads], vv[kTfHeads];
                F::sync();
                const f2 x01 = keep[0], x23 = keep[1], x45 = keep[2];
                const float x[kTfMaxModelDim] = {x01.x, x01.y, x23.x, x23.y, x45.x, x45.y};
#pragma unroll
                for (int h = 0; h < kTfHeads; ++h) {
                    q[h] = affine6(t.qkv[c][0][h][0], t.qkv[c][0][h][1], x);
                    kk[h] = affine6(t.qkv[c][1][h][0], t.qkv[c][1][h][1], x);
                    vv[h] = affine6(t.qkv[c][2][h][0], t.qkv[c][2][h][1], x);
                }
                F::sync();                                          // (the channel before has been read)
                if constexpr (Tensors::kFresh) kv = (f2*)xs + 3 * Tensors::fresh(lane);
                kv[0] = f2{kk[0], kk[1]};
                kv[1] = f2{kk[2], vv[0]};
                kv[2] = f2{vv[1], vv[2]};
                F::sync();
                const f2* rj = (const f2*)xs;
                float mx = -INFINITY;
#pragma unroll 2
                for (int j = 0; j < S; ++j) {
                    const f2 k01 = rj[3 * j], k2v = rj[3 * j + 1];
                    mx = fmaxf(mx, fmaf(q[2], k2v.x, fmaf(q[1], k01.y, q[0] * k01.x)));
                }
                float sum = 0.0f, o0 = 0.0f, o1 = 0.0f, o2 = 0.0f;
#pragma unroll 2
                for (int j = 0; j < S; ++j) {
                    const f2 k01 = rj[3 * j], k2v = rj[3 * j + 1], v12 = rj[3 * j + 2];
                    const float s = fmaf(q[2], k2v.x, fmaf(q[1], k01.y, q[0] * k01.x));
                    const float w = __builtin_amdgcn_exp2f(s - mx);
                    sum += w;
                    o0 = fmaf(w, k2v.y, o0);
                    o1 = fmaf(w, v12.x, o1);
                    o2 = fmaf(w, v12.y, o2);
                }
                const float r = 1.0f / sum;
                const float o[kTfHeads] = {o0 * r, o1 * r, o2 * r};
#pragma unroll
                for (int h = 0; h < kTfHeads; ++h) {
                    const f4 d0 = t.dn[c][h][0], d1 = t.dn[c][h][1];
                    a[0] = fmaf(d0.x, o[h], a[0]); a[1] = fmaf(d0.y, o[h], a[1]); a[2] = fmaf(d0.z, o[h], a[2]);
                    a[3] = fmaf(d0.w, o[h], a[3]); a[4] = fmaf(d1.x, o[h], a[4]); a[5] = fmaf(d1.y, o[h], a[5]);
                }
            }
            if (resid) {
                F::sync();
                const f2 x01 = keep[0], x23 = keep[1], x45 = keep[2];
                a[0] = x01.x + a[0]; a[1] = x01.y + a[1]; a[2] = x23.x + a[2]; a[3] = x23.y + a[3]; a[4] = x45.x + a[4]; a[5] = x45.y + a[5];
            }
            layer_norm(a, dm, t.vec[1][0], t.vec[1][1], t.vec[2][0], t.vec[2][1]);
            // the feed-forward network, unit by unit
            float f[kTfMaxModelDim] = {t.vec[3][0].x, t.vec[3][0].y, t.vec[3][0].z, t.vec[3][0].w, t.vec[3][1].x, t.vec[3][1].y};
#pragma unroll 2
            for (int u = 0; u < kTfFeedForward; ++u) {
                float hdn = affine6(t.ff[u][0], t.ff[u][1], a);
                hdn = hdn < 0.0f ? 0.0f : hdn;                      // relu (a NaN stays one)
                const f4 w0 = t.ff[u][2], w1 = t.ff[u][3];
                f[0] = fmaf(w0.x, hdn, f[0]); f[1] = fmaf(w0.y, hdn, f[1]); f[2] = fmaf(w0.z, hdn, f[2]);
                f[3] = fmaf(w0.w, hdn, f[3]); f[4] = fmaf(w1.x, hdn, f[4]); f[5] = fmaf(w1.y, hdn, f[5]);
            }
            if (resid) {
#pragma unroll
                for (int c = 0; c < kTfMaxModelDim; ++c) f[c] = a[c] + f[c];
            }
            layer_norm(f, dm, t.vec[4][0], t.vec[4][1], t.vec[5][0], t.vec[5][1]);
#pragma unroll
            for (int c = 0; c < kTfMaxModelDim; ++c) x[c] = f[c];
        }
        F::sync();                                                  // (every lane is done with what it kept in the y row)
        float* ys = ts.y[slot];
#pragma unroll
        for (int c = 0; c < kTfMaxModelDim; ++c)
            if (valid && c < dm) ys[lane * dm + c] = x[c];
        F::sync();
    }
};

using TransformerEncoder = TransformerEncoderOf<TransformerOwnTensors>;

// DEF: the reference's default configuration as compile-time constants (default_config_constants; bit-identical)
template <bool NORM, bool DEF>
__global__ __launch_bounds__(PolicyFamily::kBlock, 4) void k_policy_rollout_transformer(Params p, int n_steps, PolicyArgs a, NormArgs na,
                                                                                         TransformerArgs ta) {
    __shared__ PolicyFamily::Smem sm;
    __shared__ PolicySmem<false> ps;
    __shared__ TransformerSmem ts;
    if constexpr (DEF) p = default_config_constants<false>(p);
    policy_rollout_body<false, NORM, false, TransformerEncoder>(sm, ps, p, n_steps, a, na, 0, 0, TransformerEncoder{ts, ta});
}

template <bool NORM, bool DEF>
__global__ __launch_bounds__(PolicyFamily::kBlock, 4) void k_policy_evaluate_transformer(Params p, PolicyArgs a, EvalArgs ev,
                                                                                          TransformerArgs ta) {
    __shared__ PolicyFamily::Smem sm;
    __shared__ PolicySmem<false> ps;
    __shared__ EvalSmem es;
    __shared__ TransformerSmem ts;
    if constexpr (DEF) p = default_config_constants<false>(p);
    policy_evaluate_body<true, false, NORM, TransformerEncoder>(sm, &ps, es, p, a, ev, TransformerEncoder{ts, ta});
}

}  // namespace evac
