// Device code of libevac, part 7: the DEEP-SETS LEADER -- the reference's set encoder (rpo_deep_sets_agent_network.py:25-90) in
// front of the actor-critic of the policy rollout and the policy evaluation.  The Box observation is a set of S = N + 2 rows
// (pedestrians, leader, exit) of `ed` floats; the network reads
//     y = W_r . sum_i phi(x_i) + b_r,    phi(x_i) = W_b . relu(W_a x_i + b_a) + b_b,    W_a [24][ed], W_b [24][24], W_r [D][24]
// and actor_mean / critic then read y where RPOLinearNetwork reads x.  Everything below the encoder is evac_policy.h /
// evac_evaluate.h, called: the bodies take the encoder as a hook (NoEncoder there), and policy_eval takes its input row.
//
// One wave per env, as the policy kernels.  The encoder turns the wave's LDS row x into a second LDS row y in three phases:
//   A  lane = element, in passes of 64 over S (N = 63, 64: a second pass of 1 or 2 lanes).  The lane holds its element's `ed`
//      values; the 24 x (ed + 1) weights of W_a, b_a are staged ONCE per workgroup in LDS as two 16-byte vectors per unit and read
//      as broadcasts.  Three units at a time: h_k = relu(b_a[k] + sum_c W_a[k][c] x_c), c ascending, summed over the lanes by
//      wave_sum3 (a fixed tree) into t[k] = sum_i relu(..)_k; a second pass adds its sums to the first's.
//   B  the pooling is linear above the relu: sum_i phi(x_i) = W_b t + S b_b.  Lane k < 24 computes s_k = S b_b[k] + sum_j W_b[k][j] t_j,
//      j ascending (W_b staged transposed: conflict-free).  The reference applies W_b per element and then sums; this form is the
//      same function with 1/S of the multiplications and another rounding, measured against float64 in tests/test_gpu_deepsets.py.
//   C  lane j, j + 64, ... computes y_j = b_r[j] + sum_k W_r[j][k] s_k, k ascending, row j of W_r streamed from L2 as six 16-byte
//      loads (as policy_eval streams W1), s broadcast from LDS.
// Every sum has a fixed order and no atomics: the result depends on the env's observation and the weights alone.
#pragma once

#include "evac_evaluate.h"

namespace evac {

constexpr int kSetHidden = 24;                   // RPODeepSetsEmbeddingConfig.dim_hidden (the only width the kernels take)
constexpr int kSetMaxElemDim = 6;                // positions + one-hot status

// evac_deepsets_t's tensors (torch layouts, read in place)
struct DeepSetsArgs {
    const float *phi_w1, *phi_b1, *phi_w2, *phi_b2, *rho_w, *rho_b;
    int elem_dim;
};

// A population's encoders (evac_deepsets_population.h, evac_deepsets_population_evaluate.h): learner s's six tensors
struct DeepSetsStrides {
    int64_t stride[6];                          // floats from learner s to learner s + 1, in evac_deepsets_t order
};

struct DeepSetsSmem {
    alignas(16) float y[PolicyFamily::kEnvsPerBlock][kPolicyMaxObs];      // the encoded observation the actor-critic reads
    f4 wa[kSetHidden][2];                                                  // (W_a[k][0..3]), (W_a[k][4], W_a[k][5], b_a[k], -); columns >= ed are 0
    float wb[kSetHidden][kSetHidden];                                      // [j][k] = W_b[k][j]
    float bb[kSetHidden];
    alignas(16) float t[PolicyFamily::kEnvsPerBlock][2][kSetHidden];      // per wave: [0] the pooled hidden sums t, [1] s = W_b t + S b_b
    DeepSetsArgs a;                                                        // (read back where used, as PolicySmem::args)
};

struct DeepSetsEncoder {
    static constexpr bool kOn = true;
    DeepSetsSmem& ds;
    const DeepSetsArgs& ka;

    // by the whole workgroup, before the staging barrier (beside stage_policy)
    __device__ __forceinline__ void stage() const {
        const int ed = ka.elem_dim;
        for (int k = (int)threadIdx.x; k < kSetHidden; k += PolicyFamily::kBlock) {
            float w[kSetMaxElemDim];
#pragma unroll
            for (int c = 0; c < kSetMaxElemDim; ++c) w[c] = c < ed ? ka.phi_w1[k * ed + c] : 0.0f;
            ds.wa[k][0] = f4{w[0], w[1], w[2], w[3]};
            ds.wa[k][1] = f4{w[4], w[5], ka.phi_b1[k], 0.0f};
            ds.bb[k] = ka.phi_b2[k];
        }
        for (int idx = (int)threadIdx.x; idx < kSetHidden * kSetHidden; idx += PolicyFamily::kBlock) {
            const int j = idx / kSetHidden, k = idx % kSetHidden;
            ds.wb[j][k] = ka.phi_w2[k * kSetHidden + j];
        }
        if (threadIdx.x == 0) ds.a = ka;
    }

    __device__ __forceinline__ const float* row(int slot) const { return ds.y[slot]; }

    // x (the wave's LDS row of D = S x ed floats) -> y (ds.y[slot]); the caller has synchronised x, y is synchronised on return
    __device__ __forceinline__ void encode(const float* xs, int slot, int lane, int D, int S) const {
        using F = PolicyFamily;
        const int ed = ds.a.elem_dim;
        float* t = ds.t[slot][0];
        // A: the pooled hidden sums
        for (int base = 0; base < S; base += kWave) {
            const int i = base + lane;
            const bool valid = i < S;
            float x[kSetMaxElemDim];
#pragma unroll
            for (int c = 0; c < kSetMaxElemDim; ++c) x[c] = (valid && c < ed) ? xs[i * ed + c] : 0.0f;
#pragma unroll 1
            for (int k = 0; k < kSetHidden; k += 3) {
                float h[3];
#pragma unroll
                for (int u = 0; u < 3; ++u) {
                    const f4 w0 = ds.wa[k + u][0], w1 = ds.wa[k + u][1];
                    float v = w1.z;
                    v = fmaf(w0.x, x[0], v); v = fmaf(w0.y, x[1], v); v = fmaf(w0.z, x[2], v); v = fmaf(w0.w, x[3], v);
                    v = fmaf(w1.x, x[4], v); v = fmaf(w1.y, x[5], v);
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
        F::sync();
        // B: s = W_b t + S b_b
        if (lane < kSetHidden) {
            float s = (float)S * ds.bb[lane];
#pragma unroll
            for (int j = 0; j < kSetHidden; ++j) s = fmaf(ds.wb[j][lane], t[j], s);
            t[kSetHidden + lane] = s;
        }
        F::sync();
        // C: y = W_r s + b_r
        const DeepSetsArgs& a = ds.a;
        float* ys = ds.y[slot];
        const f4* sv = (const f4*)(t + kSetHidden);
#pragma unroll 1
        for (int j = lane; j < D; j += kWave) {
            const f4* __restrict__ r = (const f4*)(a.rho_w + (size_t)j * kSetHidden);
            float v = a.rho_b[j];
#pragma unroll
            for (int g = 0; g < kSetHidden / 4; ++g) {
                const f4 w = r[g], s = sv[g];
                v = fmaf(w.x, s.x, v); v = fmaf(w.y, s.y, v); v = fmaf(w.z, s.z, v); v = fmaf(w.w, s.w, v);
            }
            ys[j] = v;
        }
        F::sync();
    }
};

// DEF: the reference's default configuration as compile-time constants (default_config_constants; bit-identical)
template <bool NORM, bool DEF>
__global__ __launch_bounds__(PolicyFamily::kBlock, 4) void k_policy_rollout_deepsets(Params p, int n_steps, PolicyArgs a, NormArgs na,
                                                                                      DeepSetsArgs da) {
    __shared__ PolicyFamily::Smem sm;
    __shared__ PolicySmem<false> ps;
    __shared__ DeepSetsSmem ds;
    if constexpr (DEF) p = default_config_constants<false>(p);
    policy_rollout_body<false, NORM, false, DeepSetsEncoder>(sm, ps, p, n_steps, a, na, 0, 0, DeepSetsEncoder{ds, da});
}

template <bool NORM, bool DEF>
__global__ __launch_bounds__(PolicyFamily::kBlock, 4) void k_policy_evaluate_deepsets(Params p, PolicyArgs a, EvalArgs ev, DeepSetsArgs da) {
    __shared__ PolicyFamily::Smem sm;
    __shared__ PolicySmem<false> ps;
    __shared__ EvalSmem es;
    __shared__ DeepSetsSmem ds;
    if constexpr (DEF) p = default_config_constants<false>(p);
    policy_evaluate_body<true, false, NORM, DeepSetsEncoder>(sm, &ps, es, p, a, ev, DeepSetsEncoder{ds, da});
}

}  // namespace evac
