// Device code of libevac, part 9: the TRANSFORMER LEADER'S GRADIENT -- the RPO minibatch gradient of evac_train.h for the network
// of evac_transformer.h, all 13 + 16 per block tensors (include/evac.h: evac_transformer_minibatch_grad).  The actor-critic behind
// the encoder is differentiated by the three kernels of evac_train.h as they are, on the ENCODED observations; four kernels here
// stand around them:
//   k_tf_encode      one wave per sample, lane = token: gathers x = b_obs[inds[m]], runs the blocks as TransformerEncoder::encode
//                    does (the same formulas in the same order: j ascending, two-pass softmax in exp2, the scale folded into W_q)
//                    and leaves Y[m][D] -- and, with two blocks, the first block's output X1[m][D] -- in the workspace, with the
//                    minibatch-ordered copies of actions / logprobs / advantages / returns / values and the index vector 0..M-1.
//                    Its first workgroup clears k_tf_finish's ticket.
//   k_tf_dy          dX[m][D] = W1a^T g1a + W1c^T g1c in tiles of 8 samples (k_set_backward's first phase).
//   k_tf_backward    ONE BLOCK of the encoder, backwards; launched for the last block first.  One wave per sample, lane = token:
//                    the block's forward pass again from its input (x gathered, or X1), keeping per token o, the rows' maxima and
//                    sums in LDS and the two norms' xhat / rstd in registers; then LayerNorm2, the feed-forward network, LayerNorm1
//                    and `dense` backwards in the token's registers; then the attention one channel at a time: a ROW pass (lane =
//                    i, loop j: dq) and a COLUMN pass (lane = j, loop i with q_i, do_i, m_i, 1 / l_i, Dr_i broadcast from LDS: dk,
//                    dv), no cross-lane transposes.  The weights' gradients switch to "lane = weight row": 96 feed-forward units
//                    in two passes, 18 dense columns, 9 x 7 Q/K/V entries per channel, each lane looping over the tokens with the
//                    per-token vectors broadcast from LDS; what a sample adds goes to the WAVE'S accumulators in LDS (one
//                    read-modify-write per entry and sample, by the one lane that owns it).  The block's input gradient
//                    overwrites the sample's row of dX for the next launch.  The workgroup writes ONE partial, waves in order.
//   k_tf_finish      adds the partials in workgroup order, writes the 16 tensors of every block in use, and the last workgroup
//                    (an INTEGER ticket) adds their sums of squares to stats[7] (k_rpo_finish wrote it before this launch).
// Every sum has a fixed order, no floating-point atomics: the same bits on every run and stream.  f32 fmaf chains on the VALU
// (no MFMA: every contraction is 6 or 3 wide).
// The four are templates over an optional trailing argument, as k_rpo_* are: k_tf_*<> are evac_transformer_minibatch_grad's
// kernels; k_tf_*<const AdamHeader*> are evac_transformer_update's, which return at once, touching nothing (k_tf_encode not even
// the ticket), when the header's stop flag is set; k_tf_*<const AdamHeader*, TfgLearnerStrides> are a population's
// (evac_transformer_update_population: the learner is blockIdx.y; see TfgLearner below), instantiated by its unit alone.
#pragma once

#include "evac_train.h"

namespace evac {

constexpr int kTfgHeads = 3;                     // (evac_transformer_host.h's limits: the unit asserts them)
constexpr int kTfgFeedForward = 96;
constexpr int kTfgDm = 6;
constexpr int kTfgMaxBlocks = 2;
constexpr float kTfgLnEps = 1e-5f;
constexpr int kTfgTensors = 16;                  // per block, evac_transformer_block_t's order
constexpr int kTfgEncodeBlock = 256;             // k_tf_encode, k_tf_dy, k_tf_finish: 4 waves
constexpr int kTfgEncodeWaves = kTfgEncodeBlock / 64;
constexpr int kTfgEncodeMaxWgs = 2048;
constexpr int kTfgBlock = 128;                   // k_tf_backward: 2 waves (25 KB of LDS a wave)
constexpr int kTfgWaves = kTfgBlock / 64;
constexpr int kTfgTile = 8;                      // samples per workgroup of k_tf_dy
constexpr int kTfgSamplesPerWg = 32;
constexpr int kTfgMaxParts = 512;                // workgroups of k_tf_backward at most
constexpr int kTfgRowMax = (kTrainMaxObs + 3) & ~3;
// One workgroup's partial of one block, in floats, padded to 6 channels (k_tf_finish drops the padding):
//   Q/K/V  [c 6][r 9][e 7]   r = 3 (q | k | v) + h: the row h dm + c of W_q | W_k | W_v, e < 6 its column, e = 6 the bias
//   dense  [col 18][c' 6]    dense_w[c'][col], col = 3 c + h;   then dense_b [6]
//   ff     [n 96][13]        ff1_w[n][0..5], ff1_b[n], ff2_w[0..5][n];   then ff2_b [6]
//   norms  norm1_w, norm1_b, norm2_w, norm2_b [6] each
constexpr int kTfgQkvLanes = 9 * 7;                                        // 63
constexpr int kTfgPartQkv = 0;
constexpr int kTfgPartDense = kTfgPartQkv + kTfgDm * kTfgQkvLanes;         // 378
constexpr int kTfgPartDenseB = kTfgPartDense + 18 * kTfgDm;                // 486
constexpr int kTfgPartFf = kTfgPartDenseB + kTfgDm;                        // 492
constexpr int kTfgPartFfB = kTfgPartFf + kTfgFeedForward * 13;             // 1740
constexpr int kTfgPartNorm = kTfgPartFfB + kTfgDm;                         // 1746
constexpr int kTfgPart = kTfgPartNorm + 4 * kTfgDm;                        // 1770
constexpr int kTfgFinishWgs = 8;                 // per block
constexpr int kTfgFinishSlice = (kTfgPart + kTfgFinishWgs - 1) / kTfgFinishWgs;   // 222 entries a workgroup
constexpr int kTfgHeaderBytes = 256;             // the ticket [16 words] | slots [2 x 8] | -
static_assert(kTfgFinishSlice <= kTfgEncodeBlock, "k_tf_finish: one entry per thread");

__host__ __device__ inline int tfg_parts(int64_t M) {
    const int64_t p = (M + kTfgSamplesPerWg - 1) / kTfgSamplesPerWg;
    return (int)(p < 1 ? 1 : (p > kTfgMaxParts ? kTfgMaxParts : p));
}

struct TfgBlock {
    const float* w[kTfgTensors];                 // wq bq wk bk wv bv dense_w dense_b ff1_w ff1_b ff2_w ff2_b norm1_w norm1_b norm2_w norm2_b
    float* g[kTfgTensors];
};
struct TfgArgs {
    TfgBlock blk[kTfgMaxBlocks];
    const float *w1a, *w1c;                      // the actor's and the critic's first layer [64][D]
    const float *obs, *actions, *logprobs, *adv, *ret, *val;   // the caller's batch
    const int64_t* inds;                         // [M]
    int64_t B;
    // the workspace
    float *Y, *dX, *X1;                          // [M][D] each
    float *act_g, *lp_g, *adv_g, *ret_g, *val_g; // the minibatch in order: [M][2], [M] ...
    int64_t* ident;                              // 0 .. M-1
    const float* g1;                             // [2][M][64]: the layer-1 pre-activation gradients k_rpo_grad left
    float* parts;                                // [block][P][kTfgPart]
    unsigned* tickets;
    float* slots;
    float* stats;
    int D, M, dm, S, nb, resid;                  // S = D / dm tokens of dm floats
    int P, chunk;                                // workgroups of k_tf_backward, `chunk` samples each
};

__device__ __forceinline__ int64_t tfg_index(const int64_t* inds, int64_t B, int64_t m) {   // (indices outside the batch never leave it)
    const int64_t i = inds[m];
    return i < 0 ? 0 : (i >= B ? B - 1 : i);
}

// WHOSE tensors a kernel works on.  The lone forms: the arguments' own (TfgOwn: every pointer as the launch passed it).  The
// POPULATION form (include/evac.h: evac_transformer_update_population): the learner is blockIdx.y and `a` holds learner 0's
// pointers.  TfgArgs::blk[b] is indexed at run time, so `a` is never moved in place (a changed copy of it, or of one block's
// pointers, would be a private one and go to scratch: DESIGN.md sections 4.18, 4.19): a block's tensor gets its learner's shift
// WHERE IT IS NAMED, the stride read from the kernel-argument segment beside the pointer, and so do the fields that are no
// arrays (TfgLearner's functions: scalar multiply-adds the compiler shares between uses).  Parameters and gradients by the tensors' strides; what lies in a learner's
// workspace slice (dX, X1, g1, the partials, tickets and slots) by the slice; what the actor-critic's kernels read as ONE common
// batch of S x M rows -- Y, the gathered columns and the index list -- by the learner's M rows.  The caller's batch (obs .. val)
// is common and stays.  gridDim.x is the lone kernel's, so the ticket tests hold per learner.
struct TfgLearnerStrides {
    int64_t p[kTfgMaxBlocks][kTfgTensors], g[kTfgMaxBlocks][kTfgTensors];   // floats from learner s to s + 1: the blocks' parameters, gradients
    int64_t w1a, w1c;                           // ... the actor's and the critic's first layer
    int64_t hdr, ws;                            // bytes: the optimiser's header, the workspace slice
    int64_t inds, stats;                        // elements of perms / stats_out per learner
};
// Both name every field they may shift through a function, so that the lone forms read the arguments where they always did.
struct TfgOwn {
    const TfgArgs& a;
    __device__ __forceinline__ const float* w(const TfgBlock& B, int, int i) const { return B.w[i]; }
    __device__ __forceinline__ float* g(const TfgBlock& B, int, int i) const { return B.g[i]; }
    __device__ __forceinline__ const float* w1a() const { return a.w1a; }
    __device__ __forceinline__ const float* w1c() const { return a.w1c; }
    __device__ __forceinline__ const int64_t* inds() const { return a.inds; }
    __device__ __forceinline__ float* Y() const { return a.Y; }
    __device__ __forceinline__ float* dX() const { return a.dX; }
    __device__ __forceinline__ float* X1() const { return a.X1; }
    __device__ __forceinline__ float* act_g() const { return a.act_g; }
    __device__ __forceinline__ float* lp_g() const { return a.lp_g; }
    __device__ __forceinline__ float* adv_g() const { return a.adv_g; }
    __device__ __forceinline__ float* ret_g() const { return a.ret_g; }
    __device__ __forceinline__ float* val_g() const { return a.val_g; }
    __device__ __forceinline__ int64_t* ident() const { return a.ident; }
    __device__ __forceinline__ int64_t ident_of(int64_t m) const { return m; }
    __device__ __forceinline__ const float* g1() const { return a.g1; }
    __device__ __forceinline__ float* parts() const { return a.parts; }
    __device__ __forceinline__ unsigned* tickets() const { return a.tickets; }
    __device__ __forceinline__ float* slots() const { return a.slots; }
    __device__ __forceinline__ float* stats() const { return a.stats; }
};
template <class T>
__device__ __forceinline__ T* tfg_shift_bytes(T* p, int64_t bytes) { return (T*)((char*)p + bytes); }
struct TfgLearner {
    const TfgArgs& a;
    const TfgLearnerStrides& q;
    int64_t s;
    __device__ __forceinline__ int64_t rows() const { return s * a.M; }
    __device__ __forceinline__ int64_t slice() const { return s * q.ws; }
    __device__ __forceinline__ const float* w(const TfgBlock& B, int b, int i) const { return B.w[i] + s * q.p[b][i]; }
    __device__ __forceinline__ float* g(const TfgBlock& B, int b, int i) const { return B.g[i] + s * q.g[b][i]; }
    __device__ __forceinline__ const float* w1a() const { return a.w1a + s * q.w1a; }
    __device__ __forceinline__ const float* w1c() const { return a.w1c + s * q.w1c; }
    __device__ __forceinline__ const int64_t* inds() const { return a.inds + s * q.inds; }
    __device__ __forceinline__ float* Y() const { return a.Y + rows() * a.D; }
    __device__ __forceinline__ float* dX() const { return tfg_shift_bytes(a.dX, slice()); }
    __device__ __forceinline__ float* X1() const { return tfg_shift_bytes(a.X1, slice()); }
    __device__ __forceinline__ float* act_g() const { return a.act_g + 2 * rows(); }
    __device__ __forceinline__ float* lp_g() const { return a.lp_g + rows(); }
    __device__ __forceinline__ float* adv_g() const { return a.adv_g + rows(); }
    __device__ __forceinline__ float* ret_g() const { return a.ret_g + rows(); }
    __device__ __forceinline__ float* val_g() const { return a.val_g + rows(); }
    __device__ __forceinline__ int64_t* ident() const { return a.ident + rows(); }
    __device__ __forceinline__ int64_t ident_of(int64_t m) const { return rows() + m; }   // the learner's rows in the common index list
    __device__ __forceinline__ const float* g1() const { return tfg_shift_bytes(a.g1, slice()); }
    __device__ __forceinline__ float* parts() const { return tfg_shift_bytes(a.parts, slice()); }
    __device__ __forceinline__ unsigned* tickets() const { return tfg_shift_bytes(a.tickets, slice()); }
    __device__ __forceinline__ float* slots() const { return tfg_shift_bytes(a.slots, slice()); }
    __device__ __forceinline__ float* stats() const { return a.stats + s * q.stats; }
};
__device__ __forceinline__ TfgOwn tfg_whose(const TfgArgs& a) { return {a}; }
__device__ __forceinline__ TfgOwn tfg_whose(const TfgArgs& a, const AdamHeader*) { return {a}; }
__device__ __forceinline__ TfgLearner tfg_whose(const TfgArgs& a, const AdamHeader*, const TfgLearnerStrides& q) {
    return {a, q, (int64_t)blockIdx.y};
}
// the stop gate: the header, the learner's in a population
__device__ __forceinline__ const AdamHeader* tfg_gate(const AdamHeader* h) { return h; }
__device__ __forceinline__ const AdamHeader* tfg_gate(const AdamHeader* h, const TfgLearnerStrides& q) {
    return (const AdamHeader*)((const char*)h + (int64_t)blockIdx.y * q.hdr);
}

// A block's weights as the kernels read them (TransformerBlockSmem's layout: 8 640 bytes), every row zero-padded to 6 columns.
struct TfgBlockSmem {
    f4 qkv[kTfgDm][3][kTfgHeads][2];   // [c][q | k | v][h]: (W[h dm + c][0..3]), (W[..][4], W[..][5], b[h dm + c], 0); q's times log2(e) / sqrt(dm)
    f4 dn[kTfgDm][kTfgHeads][2];       // [c][h]: (dense_w[0..3][3 c + h]), (dense_w[4][..], dense_w[5][..], 0, 0)
    f4 ff[kTfgFeedForward][4];         // [n]: (W1[n][0..3]), (W1[n][4], W1[n][5], b1[n], 0), (W2[0..3][n]), (W2[4][n], W2[5][n], 0, 0)
    f4 vec[6][2];                      // dense_b, norm1_w, norm1_b, ff2_b, norm2_w, norm2_b
};

// by the whole workgroup of `step` threads, before a barrier: TransformerEncoder::stage for block b, `who`'s tensors
template <class Who>
__device__ __forceinline__ void tfg_stage(const Who& who, const TfgBlock& B, int b, TfgBlockSmem& t, int dm, int tid, int step) {
    const float qscale = 1.44269504088896341f / sqrtf((float)dm);
    float* qkv = (float*)t.qkv;
    for (int idx = tid; idx < kTfgDm * 3 * kTfgHeads * 8; idx += step) {
        const int e = idx & 7, r = idx >> 3, h = r % kTfgHeads, m = (r / kTfgHeads) % 3, c = r / (3 * kTfgHeads);
        float v = 0.0f;
        if (c < dm) {
            const int row = h * dm + c;
            if (e < dm) v = who.w(B, b, 2 * m)[row * dm + e];
            else if (e == 6) v = who.w(B, b, 2 * m + 1)[row];
            if (m == 0) v *= qscale;
        }
        qkv[idx] = v;
    }
    float* dn = (float*)t.dn;
    for (int idx = tid; idx < kTfgDm * kTfgHeads * 8; idx += step) {
        const int e = idx & 7, r = idx >> 3, h = r % kTfgHeads, c = r / kTfgHeads;
        dn[idx] = (c < dm && e < dm) ? who.w(B, b, 6)[e * (kTfgHeads * dm) + c * kTfgHeads + h] : 0.0f;
    }
    float* ff = (float*)t.ff;
    for (int idx = tid; idx < kTfgFeedForward * 16; idx += step) {
        const int e = idx & 15, u = idx >> 4;
        float v = 0.0f;
        if (e < 8) {
            if (e < dm) v = who.w(B, b, 8)[u * dm + e];
            else if (e == 6) v = who.w(B, b, 9)[u];
        } else if (e - 8 < dm) {
            v = who.w(B, b, 10)[(e - 8) * kTfgFeedForward + u];
        }
        ff[idx] = v;
    }
    float* vec = (float*)t.vec;
    for (int idx = tid; idx < 6 * 8; idx += step) {
        const int e = idx & 7, r = idx >> 3;
        const float* src = who.w(B, b, r == 0 ? 7 : (r == 1 ? 12 : (r == 2 ? 13 : (r == 3 ? 11 : (r == 4 ? 14 : 15)))));
        vec[idx] = e < dm ? src[e] : 0.0f;
    }
}

__device__ __forceinline__ float tfg_affine6(const f4 w0, const f4 w1, const float (&x)[kTfgDm]) {   // TransformerEncoder::affine6
    float v = w1.z;
    v = fmaf(w0.x, x[0], v); v = fmaf(w0.y, x[1], v); v = fmaf(w0.z, x[2], v); v = fmaf(w0.w, x[3], v);
    v = fmaf(w1.x, x[4], v); v = fmaf(w1.y, x[5], v);
    return v;
}
__device__ __forceinline__ float tfg_dot6(const f4 w0, const f4 w1, const float (&x)[kTfgDm]) {       // sum_c w[c] x[c], c ascending
    float v = w0.x * x[0];
    v = fmaf(w0.y, x[1], v); v = fmaf(w0.z, x[2], v); v = fmaf(w0.w, x[3], v); v = fmaf(w1.x, x[4], v); v = fmaf(w1.y, x[5], v);
    return v;
}
__device__ __forceinline__ void tfg_unpack(const f4 a, const f4 b, float (&v)[kTfgDm]) {
    v[0] = a.x; v[1] = a.y; v[2] = a.z; v[3] = a.w; v[4] = b.x; v[5] = b.y;
}

// TransformerEncoder::layer_norm, keeping xhat and rstd: v -> xhat w + b
__device__ __forceinline__ void tfg_layer_norm(float (&v)[kTfgDm], int dm, const f4 w0, const f4 w1, const f4 b0, const f4 b1,
                                               float (&xhat)[kTfgDm], float& rstd) {
    const float inv = 1.0f / (float)dm;
    const float mean = (((((v[0] + v[1]) + v[2]) + v[3]) + v[4]) + v[5]) * inv;          // (the padding adds zeros)
    float d[kTfgDm], var = 0.0f;
#pragma unroll
    for (int c = 0; c < kTfgDm; ++c) {
        d[c] = c < dm ? v[c] - mean : 0.0f;
        var = fmaf(d[c], d[c], var);
    }
    rstd = 1.0f / sqrtf(var * inv + kTfgLnEps);
    float w[kTfgDm], b[kTfgDm];
    tfg_unpack(w0, w1, w);
    tfg_unpack(b0, b1, b);
#pragma unroll
    for (int c = 0; c < kTfgDm; ++c) {
        xhat[c] = d[c] * rstd;
        v[c] = fmaf(xhat[c], w[c], b[c]);
    }
}
// its transpose: dy -> rstd (dxh - mean(dxh) - xhat mean(dxh xhat)) with dxh = dy w, the means over the dm real channels
__device__ __forceinline__ void tfg_layer_norm_backward(const float (&dy)[kTfgDm], int dm, const f4 w0, const f4 w1,
                                                        const float (&xhat)[kTfgDm], float rstd, float (&dr)[kTfgDm]) {
    const float inv = 1.0f / (float)dm;
    float w[kTfgDm], dxh[kTfgDm], s1 = 0.0f, s2 = 0.0f;
    tfg_unpack(w0, w1, w);
#pragma unroll
    for (int c = 0; c < kTfgDm; ++c) {
        dxh[c] = dy[c] * w[c];                                    // (0 in the padding: w is staged as 0 there)
        s1 += dxh[c];
        s2 = fmaf(dxh[c], xhat[c], s2);
    }
    const float m1 = s1 * inv, m2 = s2 * inv;
#pragma unroll
    for (int c = 0; c < kTfgDm; ++c) dr[c] = c < dm ? rstd * ((dxh[c] - m1) - xhat[c] * m2) : 0.0f;
}

// What the backward pass keeps of a block's forward pass, per token, in registers.
struct TfgKept {
    float xhat1[kTfgDm], u[kTfgDm], xhat2[kTfgDm], rstd1, rstd2;
};

// One block forwards for the wave's sample, lane = token: TransformerEncoder::encode's block body.  xs [64][6]: the block's input,
// zero-padded (columns >= dm and tokens >= S); kvs [64][6]: the channel's k, v.  With KEEP, o / the rows' maxima / 1 / the rows'
// sums go to os [64][18] and ml [64][12].  The caller has synchronised xs; on return `out` is the token's output row and kvs may
// still be read by other lanes (synchronise before writing it).
template <bool KEEP>
__device__ __forceinline__ void tfg_forward(const TfgBlockSmem& t, const float (*xs)[kTfgDm], float (*kvs)[kTfgDm], float (*os)[18],
                                            float (*ml)[12], int lane, int S, int dm, bool resid, float (&out)[kTfgDm], TfgKept& K) {
    const f2* xr = (const f2*)xs[lane];
    const f2 x01 = xr[0], x23 = xr[1], x45 = xr[2];
    const float x[kTfgDm] = {x01.x, x01.y, x23.x, x23.y, x45.x, x45.y};
    f2* kv = (f2*)kvs[lane];
    float a[kTfgDm];
    tfg_unpack(t.vec[0][0], t.vec[0][1], a);
#pragma unroll 1
    for (int c = 0; c < dm; ++c) {
        float q[kTfgHeads], kk[kTfgHeads], vv[kTfgHeads];
#pragma unroll
        for (int h = 0; h < kTfgHeads; ++h) {
            q[h] = tfg_affine6(t.qkv[c][0][h][0], t.qkv[c][0][h][1], x);
            kk[h] = tfg_affine6(t.qkv[c][1][h][0], t.qkv[c][1][h][1], x);
            vv[h] = tfg_affine6(t.qkv[c][2][h][0], t.qkv[c][2][h][1], x);
        }
        wave_sync();                                                // (the channel before has been read)
        kv[0] = f2{kk[0], kk[1]};
        kv[1] = f2{kk[2], vv[0]};
        kv[2] = f2{vv[1], vv[2]};
        wave_sync();
        const f2* rj = (const f2*)kvs;
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
        const float o[kTfgHeads] = {o0 * r, o1 * r, o2 * r};
        if constexpr (KEEP) {
            os[lane][c * kTfgHeads] = o[0]; os[lane][c * kTfgHeads + 1] = o[1]; os[lane][c * kTfgHeads + 2] = o[2];
            ml[lane][c] = mx;
            ml[lane][kTfgDm + c] = r;
        }
#pragma unroll
        for (int h = 0; h < kTfgHeads; ++h) {
            const f4 d0 = t.dn[c][h][0], d1 = t.dn[c][h][1];
            a[0] = fmaf(d0.x, o[h], a[0]); a[1] = fmaf(d0.y, o[h], a[1]); a[2] = fmaf(d0.z, o[h], a[2]);
            a[3] = fmaf(d0.w, o[h], a[3]); a[4] = fmaf(d1.x, o[h], a[4]); a[5] = fmaf(d1.y, o[h], a[5]);
        }
    }
    if (resid) {
#pragma unroll
        for (int c = 0; c < kTfgDm; ++c) a[c] = x[c] + a[c];
    }
    tfg_layer_norm(a, dm, t.vec[1][0], t.vec[1][1], t.vec[2][0], t.vec[2][1], K.xhat1, K.rstd1);
#pragma unroll
    for (int c = 0; c < kTfgDm; ++c) K.u[c] = a[c];
    float f[kTfgDm];
    tfg_unpack(t.vec[3][0], t.vec[3][1], f);
#pragma unroll 2
    for (int n = 0; n < kTfgFeedForward; ++n) {
        float hdn = tfg_affine6(t.ff[n][0], t.ff[n][1], a);
        hdn = hdn < 0.0f ? 0.0f : hdn;                              // relu (a NaN stays one)
        const f4 w0 = t.ff[n][2], w1 = t.ff[n][3];
        f[0] = fmaf(w0.x, hdn, f[0]); f[1] = fmaf(w0.y, hdn, f[1]); f[2] = fmaf(w0.z, hdn, f[2]);
        f[3] = fmaf(w0.w, hdn, f[3]); f[4] = fmaf(w1.x, hdn, f[4]); f[5] = fmaf(w1.y, hdn, f[5]);
    }
    if (resid) {
#pragma unroll
        for (int c = 0; c < kTfgDm; ++c) f[c] = a[c] + f[c];
    }
    tfg_layer_norm(f, dm, t.vec[4][0], t.vec[4][1], t.vec[5][0], t.vec[5][1], K.xhat2, K.rstd2);
#pragma unroll
    for (int c = 0; c < kTfgDm; ++c) out[c] = f[c];
}

// the token's row of a [M][D] matrix into the wave's LDS row, zero-padded: lane = token
__device__ __forceinline__ void tfg_load_row(const float* __restrict__ row, float (*xs)[kTfgDm], int lane, int S, int dm) {
#pragma unroll
    for (int c = 0; c < kTfgDm; ++c) xs[lane][c] = (lane < S && c < dm) ? row[lane * dm + c] : 0.0f;
}
__device__ __forceinline__ void tfg_store_row(float* __restrict__ row, const float (&v)[kTfgDm], int lane, int S, int dm) {
#pragma unroll
    for (int c = 0; c < kTfgDm; ++c)
        if (lane < S && c < dm) row[lane * dm + c] = v[c];
}

struct TfgEncodeWave {
    alignas(16) float x[64][kTfgDm];
    alignas(16) float kv[64][kTfgDm];
};

template <class... Gate>
__global__ __launch_bounds__(kTfgEncodeBlock) void k_tf_encode(TfgArgs a, Gate... gate) {
    if constexpr (sizeof...(Gate) != 0) {
        if (rpo_stopped(tfg_gate(gate...))) return;
    }
    const auto who = tfg_whose(a, gate...);
    __shared__ TfgBlockSmem ts[kTfgMaxBlocks];
    __shared__ TfgEncodeWave ws[kTfgEncodeWaves];
    const int tid = (int)threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int D = a.D, M = a.M, dm = a.dm, S = a.S, nb = a.nb;
    const bool resid = a.resid != 0;
    if (blockIdx.x == 0 && tid < 16) who.tickets()[tid] = 0u;
    for (int b = 0; b < nb; ++b) tfg_stage(who, a.blk[b], b, ts[b], dm, tid, kTfgEncodeBlock);
    __syncthreads();
    TfgEncodeWave& w = ws[wave];
#pragma unroll 1
    for (int64_t m = (int64_t)blockIdx.x * kTfgEncodeWaves + wave; m < M; m += (int64_t)gridDim.x * kTfgEncodeWaves) {   // (M up to 2^31 - 1)
        const int64_t idx = tfg_index(who.inds(), a.B, m);
        tfg_load_row(a.obs + (size_t)idx * (size_t)D, w.x, lane, S, dm);
        if (lane < 2) who.act_g()[2 * (size_t)m + lane] = a.actions[2 * (size_t)idx + lane];
        else if (lane == 2) who.lp_g()[m] = a.logprobs[idx];
        else if (lane == 3) who.adv_g()[m] = a.adv[idx];
        else if (lane == 4) who.ret_g()[m] = a.ret[idx];
        else if (lane == 5) who.val_g()[m] = a.val[idx];
        else if (lane == 6) who.ident()[m] = who.ident_of((int64_t)m);
        wave_sync();
        float out[kTfgDm];
        TfgKept kept;
#pragma unroll 1
        for (int b = 0; b < nb; ++b) {
            tfg_forward<false>(ts[b], w.x, w.kv, nullptr, nullptr, lane, S, dm, resid, out, kept);
            if (b + 1 < nb) {
                tfg_store_row(who.X1() + (size_t)m * (size_t)D, out, lane, S, dm);
                wave_sync();
#pragma unroll
                for (int c = 0; c < kTfgDm; ++c) w.x[lane][c] = (lane < S && c < dm) ? out[c] : 0.0f;
                wave_sync();
            }
        }
        tfg_store_row(who.Y() + (size_t)m * (size_t)D, out, lane, S, dm);
        wave_sync();
    }
}

// dX[m][j] = sum_k W1a[k][j] g1a[m][k] + sum_k W1c[k][j] g1c[m][k], k ascending, the actor first: one tile of 8 samples a workgroup
template <class... Gate>
__global__ __launch_bounds__(kTfgEncodeBlock) void k_tf_dy(TfgArgs a, Gate... gate) {
    if constexpr (sizeof...(Gate) != 0) {
        if (rpo_stopped(tfg_gate(gate...))) return;
    }
    const auto who = tfg_whose(a, gate...);
    constexpr int H1 = kTrainHidden;
    __shared__ __attribute__((aligned(16))) float gs[2 * H1][kTfgTile];        // g1 of the tile's samples: [net, unit][sample]
    const int tid = (int)threadIdx.x;
    const int D = a.D, M = a.M;
#pragma unroll 1
    for (int64_t t0 = blockIdx.x; t0 * kTfgTile < M; t0 += gridDim.x) {
        const int m0 = (int)(t0 * kTfgTile);
        const int nq = M - m0 < kTfgTile ? M - m0 : kTfgTile;
        for (int i = tid; i < 2 * H1 * kTfgTile; i += kTfgEncodeBlock) {
            const int q = i / (2 * H1), r = i - q * (2 * H1);
            const int net = r / H1, k = r - net * H1;
            gs[r][q] = q < nq ? who.g1()[((size_t)net * (size_t)M + (size_t)(m0 + q)) * H1 + k] : 0.0f;
        }
        __syncthreads();
#pragma unroll 1
        for (int j = tid; j < D; j += kTfgEncodeBlock) {
            float acc[kTfgTile];
#pragma unroll
            for (int q = 0; q < kTfgTile; ++q) acc[q] = 0.0f;
#pragma unroll 1
            for (int net = 0; net < 2; ++net) {
                const float* __restrict__ w1 = (net == 0 ? who.w1a() : who.w1c()) + j;
#pragma unroll 8
                for (int k = 0; k < H1; ++k) {
                    const float w = w1[(size_t)k * (size_t)D];
                    const f4 g0 = *(const f4*)&gs[net * H1 + k][0], g1 = *(const f4*)&gs[net * H1 + k][4];
                    acc[0] = fmaf(w, g0.x, acc[0]); acc[1] = fmaf(w, g0.y, acc[1]); acc[2] = fmaf(w, g0.z, acc[2]); acc[3] = fmaf(w, g0.w, acc[3]);
                    acc[4] = fmaf(w, g1.x, acc[4]); acc[5] = fmaf(w, g1.y, acc[5]); acc[6] = fmaf(w, g1.z, acc[6]); acc[7] = fmaf(w, g1.w, acc[7]);
                }
            }
#pragma unroll
            for (int q = 0; q < kTfgTile; ++q)
                if (q < nq) who.dX()[(size_t)(m0 + q) * (size_t)D + j] = acc[q];
        }
        __syncthreads();
    }
}

// A wave's LDS of k_tf_backward: 72 floats a token and its accumulators.
struct TfgWave {
    alignas(16) float x[64][kTfgDm];             // the block's input
    alignas(16) float kv[64][kTfgDm];            // the channel's k, v
    alignas(16) float info[64][12];              // the column pass's (qs[3], do[3], max, 1 / sum, Dr); then (dq[3], dk[3], dv[3])
    alignas(16) float u[64][kTfgDm], df[64][kTfgDm], da[64][kTfgDm];
    float o[64][18];                             // [i][3 c + h]
    float ml[64][12];                            // [i][c]: the row's maximum, [i][6 + c]: 1 / the row's sum
    float acc[kTfgPart];                         // what the wave's samples add to the block's tensors
};
static_assert(sizeof(TfgBlockSmem) + kTfgWaves * sizeof(TfgWave) <= 64 * 1024, "k_tf_backward: static LDS");

// three wave sums into the wave's accumulators at acc[0], acc[1], acc[2] (the totals are wave-uniform: lane 0 adds them)
__device__ __forceinline__ void tfg_add_sums3(float* acc, float s0, float s1, float s2, int lane) {
    wave_sum3(s0, s1, s2);
    if (lane == 0) {
        acc[0] += s0; acc[1] += s1; acc[2] += s2;
    }
}
__device__ __forceinline__ void tfg_add_sums6(float* acc, const float (&v)[kTfgDm], int lane) {
    tfg_add_sums3(acc, v[0], v[1], v[2], lane);
    tfg_add_sums3(acc + 3, v[3], v[4], v[5], lane);
}

template <class... Gate>
__global__ __launch_bounds__(kTfgBlock) void k_tf_backward(TfgArgs a, int b, Gate... gate) {
    if constexpr (sizeof...(Gate) != 0) {
        if (rpo_stopped(tfg_gate(gate...))) return;
    }
    const auto who = tfg_whose(a, gate...);
    __shared__ TfgBlockSmem t;
    __shared__ TfgWave wv[kTfgWaves];
    const int tid = (int)threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int D = a.D, M = a.M, dm = a.dm, S = a.S;
    const bool resid = a.resid != 0, valid = lane < S;
    tfg_stage(who, a.blk[b], b, t, dm, tid, kTfgBlock);
    TfgWave& w = wv[wave];
    for (int e = lane; e < kTfgPart; e += 64) w.acc[e] = 0.0f;
    __syncthreads();
    const float inv_sqrt_dm = 1.0f / sqrtf((float)dm);
    constexpr float kLn2 = 0.693147180559945309f;
    const int64_t m_begin = (int64_t)blockIdx.x * a.chunk;
    const int64_t m_end = m_begin + a.chunk < M ? m_begin + a.chunk : M;
#pragma unroll 1
    for (int64_t m = m_begin + wave; m < m_end; m += kTfgWaves) {
        // the block's input and the gradient of its output, this token's
        const float* __restrict__ xin = b == 0 ? a.obs + (size_t)tfg_index(who.inds(), a.B, m) * (size_t)D : who.X1() + (size_t)m * (size_t)D;
        float* __restrict__ dxr = who.dX() + (size_t)m * (size_t)D;
        tfg_load_row(xin, w.x, lane, S, dm);
        float dout[kTfgDm];
#pragma unroll
        for (int c = 0; c < kTfgDm; ++c) dout[c] = (valid && c < dm) ? dxr[lane * dm + c] : 0.0f;
        wave_sync();
        float out[kTfgDm];
        TfgKept K;
        tfg_forward<true>(t, w.x, w.kv, w.o, w.ml, lane, S, dm, resid, out, K);
        // LayerNorm2: d norm2_w += sum_i dout xhat2, d norm2_b += sum_i dout
        {
            float p[kTfgDm];
#pragma unroll
            for (int c = 0; c < kTfgDm; ++c) p[c] = dout[c] * K.xhat2[c];
            tfg_add_sums6(w.acc + kTfgPartNorm + 2 * kTfgDm, p, lane);
            tfg_add_sums6(w.acc + kTfgPartNorm + 3 * kTfgDm, dout, lane);
        }
        float df[kTfgDm];
        tfg_layer_norm_backward(dout, dm, t.vec[4][0], t.vec[4][1], K.xhat2, K.rstd2, df);
        tfg_add_sums6(w.acc + kTfgPartFfB, df, lane);                                       // d ff2_b
        // the feed-forward network, unit by unit: du = W1^T ([pre > 0] W2^T df)
        float du[kTfgDm];
#pragma unroll
        for (int c = 0; c < kTfgDm; ++c) du[c] = 0.0f;
#pragma unroll 2
        for (int n = 0; n < kTfgFeedForward; ++n) {
            const f4 w0 = t.ff[n][0], w1 = t.ff[n][1];
            const float pre = tfg_affine6(w0, w1, K.u);
            const float g = tfg_dot6(t.ff[n][2], t.ff[n][3], df);
            const float dh = pre > 0.0f ? g : 0.0f;
            du[0] = fmaf(w0.x, dh, du[0]); du[1] = fmaf(w0.y, dh, du[1]); du[2] = fmaf(w0.z, dh, du[2]);
            du[3] = fmaf(w0.w, dh, du[3]); du[4] = fmaf(w1.x, dh, du[4]); du[5] = fmaf(w1.y, dh, du[5]);
        }
        if (resid) {
#pragma unroll
            for (int c = 0; c < kTfgDm; ++c) du[c] = du[c] + df[c];
        }
        // LayerNorm1
        {
            float p[kTfgDm];
#pragma unroll
            for (int c = 0; c < kTfgDm; ++c) p[c] = du[c] * K.xhat1[c];
            tfg_add_sums6(w.acc + kTfgPartNorm, p, lane);
            tfg_add_sums6(w.acc + kTfgPartNorm + kTfgDm, du, lane);
        }
        float da[kTfgDm];
        tfg_layer_norm_backward(du, dm, t.vec[1][0], t.vec[1][1], K.xhat1, K.rstd1, da);
        tfg_add_sums6(w.acc + kTfgPartDenseB, da, lane);                                    // d dense_b
        {
            f2* pu = (f2*)w.u[lane];
            f2* pf = (f2*)w.df[lane];
            f2* pa = (f2*)w.da[lane];
            pu[0] = f2{K.u[0], K.u[1]}; pu[1] = f2{K.u[2], K.u[3]}; pu[2] = f2{K.u[4], K.u[5]};
            pf[0] = f2{df[0], df[1]}; pf[1] = f2{df[2], df[3]}; pf[2] = f2{df[4], df[5]};
            pa[0] = f2{da[0], da[1]}; pa[1] = f2{da[2], da[3]}; pa[2] = f2{da[4], da[5]};
        }
        wave_sync();
        // the feed-forward weights, lane = unit, two passes: the mask again from u
#pragma unroll 1
        for (int pass = 0; pass < 2; ++pass) {
            const int n = pass * 64 + lane;
            const bool on = n < kTfgFeedForward;
            const int nn = on ? n : kTfgFeedForward - 1;
            const f4 w0 = t.ff[nn][0], w1 = t.ff[nn][1], v0 = t.ff[nn][2], v1 = t.ff[nn][3];
            float gw1[kTfgDm], gw2[kTfgDm], gb1 = 0.0f;
#pragma unroll
            for (int c = 0; c < kTfgDm; ++c) gw1[c] = gw2[c] = 0.0f;
#pragma unroll 2
            for (int i = 0; i < S; ++i) {
                const f2* pu = (const f2*)w.u[i];
                const f2* pf = (const f2*)w.df[i];
                const f2 u01 = pu[0], u23 = pu[1], u45 = pu[2], f01 = pf[0], f23 = pf[1], f45 = pf[2];
                const float ui[kTfgDm] = {u01.x, u01.y, u23.x, u23.y, u45.x, u45.y};
                const float fi[kTfgDm] = {f01.x, f01.y, f23.x, f23.y, f45.x, f45.y};
                const float pre = tfg_affine6(w0, w1, ui);
                const float hdn = pre < 0.0f ? 0.0f : pre;
                const float dh = pre > 0.0f ? tfg_dot6(v0, v1, fi) : 0.0f;
                gb1 += dh;
#pragma unroll
                for (int c = 0; c < kTfgDm; ++c) {
                    gw2[c] = fmaf(fi[c], hdn, gw2[c]);
                    gw1[c] = fmaf(dh, ui[c], gw1[c]);
                }
            }
            if (on) {
                float* dst = w.acc + kTfgPartFf + n * 13;
#pragma unroll
                for (int c = 0; c < kTfgDm; ++c) {
                    dst[c] += gw1[c];
                    dst[7 + c] += gw2[c];
                }
                dst[6] += gb1;
            }
        }
        // dense: lane = column 3 c + h
        if (lane < kTfgHeads * dm) {                                // (columns of channels >= dm: o is never written there)
            float g[kTfgDm];
#pragma unroll
            for (int c = 0; c < kTfgDm; ++c) g[c] = 0.0f;
#pragma unroll 2
            for (int i = 0; i < S; ++i) {
                const float oi = w.o[i][lane];
                const f2* pa = (const f2*)w.da[i];
                const f2 a01 = pa[0], a23 = pa[1], a45 = pa[2];
                g[0] = fmaf(a01.x, oi, g[0]); g[1] = fmaf(a01.y, oi, g[1]); g[2] = fmaf(a23.x, oi, g[2]);
                g[3] = fmaf(a23.y, oi, g[3]); g[4] = fmaf(a45.x, oi, g[4]); g[5] = fmaf(a45.y, oi, g[5]);
            }
            float* dst = w.acc + kTfgPartDense + lane * kTfgDm;
#pragma unroll
            for (int c = 0; c < kTfgDm; ++c) dst[c] += g[c];
        }
        // the attention, one channel at a time
        float dx[kTfgDm];
#pragma unroll
        for (int c = 0; c < kTfgDm; ++c) dx[c] = 0.0f;
        const int qr = lane / 7, qe = lane - qr * 7;                // the Q/K/V weights' layout: lane = 7 r + e
#pragma unroll 1
        for (int c = 0; c < dm; ++c) {
            const f2* xr = (const f2*)w.x[lane];
            const f2 x01 = xr[0], x23 = xr[1], x45 = xr[2];
            const float x[kTfgDm] = {x01.x, x01.y, x23.x, x23.y, x45.x, x45.y};
            float qs[kTfgHeads], kk[kTfgHeads], vv[kTfgHeads], dov[kTfgHeads];
#pragma unroll
            for (int h = 0; h < kTfgHeads; ++h) {
                qs[h] = tfg_affine6(t.qkv[c][0][h][0], t.qkv[c][0][h][1], x);
                kk[h] = tfg_affine6(t.qkv[c][1][h][0], t.qkv[c][1][h][1], x);
                vv[h] = tfg_affine6(t.qkv[c][2][h][0], t.qkv[c][2][h][1], x);
                dov[h] = tfg_dot6(t.dn[c][h][0], t.dn[c][h][1], da);                         // do[i][c][h] = sum_c' Wd[c'][3 c + h] da_c'
            }
            const float mx = w.ml[lane][c], rl = w.ml[lane][kTfgDm + c];
            const float Dr = fmaf(dov[2], w.o[lane][c * 3 + 2], fmaf(dov[1], w.o[lane][c * 3 + 1], dov[0] * w.o[lane][c * 3]));
            wave_sync();                                            // (the channel before is done with kv and info)
            {
                f2* kv = (f2*)w.kv[lane];
                kv[0] = f2{kk[0], kk[1]};
                kv[1] = f2{kk[2], vv[0]};
                kv[2] = f2{vv[1], vv[2]};
                f4* in = (f4*)w.info[lane];
                in[0] = f4{qs[0], qs[1], qs[2], dov[0]};
                in[1] = f4{dov[1], dov[2], mx, rl};
                in[2] = f4{Dr, 0.0f, 0.0f, 0.0f};
            }
            wave_sync();
            // the row pass, lane = i: ds_ij = w_ij (dw_ij - Dr_i), dq_i = sum_j ds_ij k_j
            float dq[kTfgHeads] = {0.0f, 0.0f, 0.0f};
            const f2* rj = (const f2*)w.kv;
#pragma unroll 2
            for (int j = 0; j < S; ++j) {
                const f2 k01 = rj[3 * j], k2v = rj[3 * j + 1], v12 = rj[3 * j + 2];
                const float s = fmaf(qs[2], k2v.x, fmaf(qs[1], k01.y, qs[0] * k01.x));
                const float wij = __builtin_amdgcn_exp2f(s - mx) * rl;
                const float dw = fmaf(dov[2], v12.y, fmaf(dov[1], v12.x, dov[0] * k2v.y));
                const float ds = wij * (dw - Dr);
                dq[0] = fmaf(ds, k01.x, dq[0]); dq[1] = fmaf(ds, k01.y, dq[1]); dq[2] = fmaf(ds, k2v.x, dq[2]);
            }
            // the column pass, lane = j: dv_j = sum_i w_ij do_i, dk_j = sum_i ds_ij q_i
            float dk[kTfgHeads] = {0.0f, 0.0f, 0.0f}, dv[kTfgHeads] = {0.0f, 0.0f, 0.0f};
            const f4* ri = (const f4*)w.info;
#pragma unroll 2
            for (int i = 0; i < S; ++i) {
                const f4 i0 = ri[3 * i], i1 = ri[3 * i + 1];
                const float Dri = w.info[i][8];
                const float s = fmaf(i0.z, kk[2], fmaf(i0.y, kk[1], i0.x * kk[0]));
                const float wij = __builtin_amdgcn_exp2f(s - i1.z) * i1.w;
                const float dw = fmaf(i1.y, vv[2], fmaf(i1.x, vv[1], i0.w * vv[0]));
                const float ds = wij * (dw - Dri);
                dv[0] = fmaf(wij, i0.w, dv[0]); dv[1] = fmaf(wij, i1.x, dv[1]); dv[2] = fmaf(wij, i1.y, dv[2]);
                dk[0] = fmaf(ds, i0.x, dk[0]); dk[1] = fmaf(ds, i0.y, dk[1]); dk[2] = fmaf(ds, i0.z, dk[2]);
            }
            // qs = q log2(e) / sqrt(dm): dq = sum ds k / sqrt(dm); dk = sum ds q / sqrt(dm) = ln 2 sum ds qs; and the staged W_q
            // is W_q log2(e) / sqrt(dm): dq W_q = ln 2 (sum ds k) W_q'
            float gq[kTfgHeads], gqx[kTfgHeads], gk[kTfgHeads], gv[kTfgHeads];
#pragma unroll
            for (int h = 0; h < kTfgHeads; ++h) {
                gq[h] = valid ? dq[h] * inv_sqrt_dm : 0.0f;
                gqx[h] = valid ? dq[h] * kLn2 : 0.0f;
                gk[h] = valid ? dk[h] * kLn2 : 0.0f;
                gv[h] = valid ? dv[h] : 0.0f;
            }
#pragma unroll
            for (int h = 0; h < kTfgHeads; ++h) {
                float wq[kTfgDm], wk[kTfgDm], wvv[kTfgDm];
                tfg_unpack(t.qkv[c][0][h][0], t.qkv[c][0][h][1], wq);
                tfg_unpack(t.qkv[c][1][h][0], t.qkv[c][1][h][1], wk);
                tfg_unpack(t.qkv[c][2][h][0], t.qkv[c][2][h][1], wvv);
#pragma unroll
                for (int e = 0; e < kTfgDm; ++e) {
                    dx[e] = fmaf(gqx[h], wq[e], dx[e]);
                    dx[e] = fmaf(gk[h], wk[e], dx[e]);
                    dx[e] = fmaf(gv[h], wvv[e], dx[e]);
                }
            }
            wave_sync();                                            // (every lane has read info)
            {
                f4* in = (f4*)w.info[lane];
                in[0] = f4{gq[0], gq[1], gq[2], gk[0]};
                in[1] = f4{gk[1], gk[2], gv[0], gv[1]};
                in[2] = f4{gv[2], 0.0f, 0.0f, 0.0f};
            }
            wave_sync();
            // the rows h dm + c of W_q, W_k, W_v and their biases: lane = 7 r + e, over the tokens
            if (lane < kTfgQkvLanes) {
                float g = 0.0f;
#pragma unroll 4
                for (int i = 0; i < S; ++i) {
                    const float xe = qe < kTfgDm ? w.x[i][qe] : 1.0f;
                    g = fmaf(w.info[i][qr], xe, g);
                }
                w.acc[kTfgPartQkv + c * kTfgQkvLanes + lane] += g;
            }
        }
        if (resid) {
#pragma unroll
            for (int c = 0; c < kTfgDm; ++c) dx[c] = dx[c] + da[c];
        }
        if (b > 0) tfg_store_row(dxr, dx, lane, S, dm);
        wave_sync();                                                // (the next sample overwrites the wave's rows)
    }
    // the workgroup's partial: per entry the waves in wave order
    __syncthreads();
    float* part = who.parts() + ((size_t)b * (size_t)a.P + (size_t)blockIdx.x) * kTfgPart;
    for (int e = tid; e < kTfgPart; e += kTfgBlock) {
        float s = 0.0f;
#pragma unroll
        for (int k = 0; k < kTfgWaves; ++k) s += wv[k].acc[e];
        part[e] = s;
    }
}

// where entry e of a block's partial goes: the tensor (0..15) and the offset in it, or tensor -1 for the padding
__device__ __forceinline__ int tfg_entry(int e, int dm, int& off) {
    if (e < kTfgPartDense) {
        const int c = e / kTfgQkvLanes, l = e - c * kTfgQkvLanes, r = l / 7, ee = l - r * 7, m = r / 3, h = r - m * 3;
        if (c >= dm) return -1;
        const int row = h * dm + c;
        if (ee == 6) return off = row, 2 * m + 1;
        if (ee >= dm) return -1;
        return off = row * dm + ee, 2 * m;
    }
    if (e < kTfgPartDenseB) {
        const int k = e - kTfgPartDense, col = k / kTfgDm, c2 = k - col * kTfgDm, c = col / 3, h = col - c * 3;
        if (c >= dm || c2 >= dm) return -1;
        return off = c2 * (kTfgHeads * dm) + c * kTfgHeads + h, 6;
    }
    if (e < kTfgPartFf) {
        const int c = e - kTfgPartDenseB;
        return c < dm ? (off = c, 7) : -1;
    }
    if (e < kTfgPartFfB) {
        const int k = e - kTfgPartFf, n = k / 13, j = k - n * 13;
        if (j < 6) return j < dm ? (off = n * dm + j, 8) : -1;
        if (j == 6) return off = n, 9;
        return j - 7 < dm ? (off = (j - 7) * kTfgFeedForward + n, 10) : -1;
    }
    if (e < kTfgPartNorm) {
        const int c = e - kTfgPartFfB;
        return c < dm ? (off = c, 11) : -1;
    }
    const int k = e - kTfgPartNorm, which = k / kTfgDm, c = k - which * kTfgDm;
    return c < dm ? (off = c, 12 + which) : -1;
}

template <class... Gate>
__global__ __launch_bounds__(kTfgEncodeBlock) void k_tf_finish(TfgArgs a, Gate... gate) {
    if constexpr (sizeof...(Gate) != 0) {
        if (rpo_stopped(tfg_gate(gate...))) return;
    }
    const auto who = tfg_whose(a, gate...);
    __shared__ float buf[kTfgEncodeBlock];
    __shared__ float fin[kTfgMaxBlocks * kTfgFinishWgs];
    __shared__ int last;
    const int tid = (int)threadIdx.x;
    const int b = (int)blockIdx.x / kTfgFinishWgs, slice = (int)blockIdx.x - b * kTfgFinishWgs;
    const int P = a.P, dm = a.dm;
    const int e = slice * kTfgFinishSlice + tid;
    float sq = 0.0f;
    if (tid < kTfgFinishSlice && e < kTfgPart) {
        int off = 0;
        const int tensor = tfg_entry(e, dm, off);
        if (tensor >= 0) {                                          // the partials of k_tf_backward in workgroup order
            const float* src = who.parts() + (size_t)b * (size_t)P * kTfgPart + e;
            float s = 0.0f;
#pragma unroll 8
            for (int p = 0; p < P; ++p) s += src[(size_t)p * kTfgPart];
            who.g(a.blk[b], b, tensor)[off] = s;
            sq = s * s;
        }
    }
    // the workgroup's sum of squares: a fixed tree
    buf[tid] = sq;
    __syncthreads();
#pragma unroll 1
    for (int s = kTfgEncodeBlock / 2; s > 0; s >>= 1) {
        if (tid < s) buf[tid] += buf[tid + s];
        __syncthreads();
    }
    if (tid == 0) who.slots()[blockIdx.x] = buf[0];
    __threadfence();                           // (release: every thread's stores, before the workgroup takes its ticket)
    __syncthreads();
    if (tid == 0) last = atomicAdd(who.tickets(), 1u) == gridDim.x - 1u;
    __syncthreads();
    if (!last) return;
    __threadfence();
    // the last workgroup to finish: the encoder's sum of squares joins the 13 tensors' (k_rpo_finish wrote stats[7] before this launch)
    if (tid < kTfgMaxBlocks * kTfgFinishWgs) fin[tid] = tid < (int)gridDim.x ? who.slots()[tid] : 0.0f;
    __syncthreads();
    if (tid == 0) {
        float s = 0.0f;
#pragma unroll
        for (int i = 0; i < kTfgMaxBlocks * kTfgFinishWgs; ++i) s += fin[i];
        who.stats()[7] = who.stats()[7] + s;
    }
}

}  // namespace evac
