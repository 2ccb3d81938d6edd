// Device code of libevac, part 5: the POLICY ROLLOUT -- the collection phase of the reference trainer (rpo_agent.py:180-196) in
// one launch: per step the actor-critic of RPOLinearNetwork (rpo_linear_agent_network.py:19-61) reads the observation, samples
// the action on the device, and the env steps with it -- the same step body (step_env), reset, episode records and
// normalisation chain as evac_step_normalized / evac_step, so the env side is bit-identical to stepping with the recorded actions.
//
// One wave per env (N <= 64), in CU-wide workgroups of 16 envs.  Lane k computes hidden unit k of every layer:
//   layer 1   h1_k = tanh(b1_k + sum_j W1[k][j] x_j)      x from the wave's LDS row (broadcast reads); the gravity observation's
//                                                         6 x 64 weights are staged in LDS, generic observations stream W1 from L2
//   layer 2   h2_k = tanh(b2_k + sum_j W2[k][j] h1_j)     W2 of actor and critic staged ONCE per workgroup in LDS as
//                                                         [j / 4][k] 16-byte vectors (conflict-free), h1 broadcast from LDS
//   layer 3   mu_0, mu_1, value = sums over the lanes     one wave_sum3 (a fixed tree)
// The actor and the critic run side by side (the critic is not on the env's dependency chain; its instructions fill the actor's
// latencies).  The policy noise of 64 steps is drawn at once, one step per lane (as the RandomAgent actions of rollout_body),
// and read back per step from LDS.  No new register state beside the step's: 113-127 VGPRs, no scratch (tools/kernel_resources.py).
#pragma once

#include "evac_device.h"

namespace evac {

constexpr uint32_t kStreamPolicy = 0x504f4c49u;  // 'POLI': the policy's Gaussian noise (Philox counter word 3)
constexpr int kHidden = 64;                      // RPOLinearNetworkConfig.num_hidden (the only width the kernel takes)
constexpr int kPolicyMaxObs = 396;               // (64 + 2) x 6: Box + ohe at N = 64, the widest observation of a one-wave env

// evac_mlp_policy_t's tensors (torch layouts: W [out][in] row-major, b [out]) and the caller's storage
struct PolicyArgs {
    const float *aw1, *ab1, *aw2, *ab2, *aw3, *ab3, *logstd;
    const float *cw1, *cb1, *cw2, *cb2, *cw3, *cb3;
    float *next_obs, *next_done;                                  // [E][D], [E]: in / out
    float *obs_out, *actions_out, *logprob_out, *value_out;       // [T][E][D], [T][E][2], [T][E], [T][E]
    float *reward_out, *done_out, *next_value_out;                // [T][E], [T][E], [E]
    evac_episode_stats_t* final_stats;                            // [T][E] or NULL
};

using PolicyFamily = Wave<1, 1024>;

// The network's weights live in LDS, staged ONCE per workgroup (the step's state leaves no registers for them: the rollout
// kernels are at 121-125 VGPRs of 128), as 16-byte vectors that a wave reads without bank conflicts: lane k reads entry [.][k].
template <bool GRAV>
struct PolicySmem {
    f4 w2[2][kHidden / 4][kHidden];                                                   // [actor | critic][j / 4][k] = W2[k][4 j/4 .. +3]
    f4 w1[GRAV ? 2 : 1][2][GRAV ? kHidden : 1];                                       // gravity observation: [actor | critic][j / 4][k] = W1[k][..], 0-padded
    f4 unit[2][kHidden];                                                              // [0][k] = (b1[k], b2[k]) of actor, critic; [1][k] = W3 column k
    alignas(16) float h[PolicyFamily::kEnvsPerBlock][2][kHidden];                     // layer-1 activations of each wave's env
    alignas(16) float x[PolicyFamily::kEnvsPerBlock][GRAV ? 8 : kPolicyMaxObs];       // the observation the policy reads
    float2 z[PolicyFamily::kEnvsPerBlock][kWave];                                      // the policy noise of 64 steps, by step
    // The launch's arguments and the policy's uniform constants, read back where they are used: the fence of every LDS hand-off
    // keeps the compiler from holding them in scalar registers through the step, which already takes them all
    PolicyArgs args;
    NormArgs na;
    f4 c[3];                                                                           // (b3 actor 0, 1, b3 critic, -), (sigma, sigma^2), (log sigma, -)
};

// The raw observation of the env (write_obs_generic's per-lane mapping) into the wave's LDS row; the normalisation chain then
// runs over that row with lane j % 64 owning feature j -- the same owner for the terminal and the reset observation, so the two
// updates of a feature stay ordered, and the norm_state / storage accesses are coalesced.
struct StoreStage {
    float* x;
    __device__ __forceinline__ void operator()(int idx, float v) const { x[idx] = v; }
};
template <bool GRAV, class F>
__device__ __forceinline__ void stage_observation(const Params& p, typename F::Ctx& w, bool active, const Ped& q, const Env& e,
                                                  const float (&o6)[6], float* xs) {
    if constexpr (GRAV) {
        if (w.i < 6) {
            float v = o6[0];
#pragma unroll
            for (int j = 1; j < 6; ++j) v = w.i == j ? o6[j] : v;
            xs[w.i] = v;
        }
    } else {
        write_obs_generic(p, w.i, active, q, e, StoreStage{xs});
    }
    F::sync();
}

// actor_mean(x) and critic(x) of the observation in the wave's LDS row (every lane computes unit `k` = its lane; results
// wave-uniform, b3 not added).  ACTOR = false: the critic alone (the bootstrap value).  CRITIC = false: the actor alone (the
// policy evaluation, which has no use for values; v comes back 0).  `row`: the LDS row the first layer reads instead of the
// observation's (an encoder's output: evac_deepsets.h).
template <bool GRAV, bool ACTOR, bool CRITIC = true>
__device__ __forceinline__ void policy_eval(const PolicyArgs& a, PolicySmem<GRAV>& ps, int slot, int k, int D, float& m0, float& m1,
                                            float& v, const float* row = nullptr) {
    const float* xs = row ? row : ps.x[slot];
    const f4 u0 = ps.unit[0][k];
    float ha = u0.x, hc = u0.y;
    if constexpr (GRAV) {
        const f4 x03 = *(const f4*)xs;
        const f2 x45 = *(const f2*)(xs + 4);
        f4 wc0{}, wc1{};
        if constexpr (CRITIC) {
            wc0 = ps.w1[1][0][k];
            wc1 = ps.w1[1][1][k];
        }
        if constexpr (ACTOR) {
            const f4 wa0 = ps.w1[0][0][k], wa1 = ps.w1[0][1][k];
            ha = fmaf(wa0.x, x03.x, ha); ha = fmaf(wa0.y, x03.y, ha); ha = fmaf(wa0.z, x03.z, ha); ha = fmaf(wa0.w, x03.w, ha);
            ha = fmaf(wa1.x, x45.x, ha); ha = fmaf(wa1.y, x45.y, ha);
        }
        if constexpr (CRITIC) {
            hc = fmaf(wc0.x, x03.x, hc); hc = fmaf(wc0.y, x03.y, hc); hc = fmaf(wc0.z, x03.z, hc); hc = fmaf(wc0.w, x03.w, hc);
            hc = fmaf(wc1.x, x45.x, hc); hc = fmaf(wc1.y, x45.y, hc);
        }
    } else {
        const float* __restrict__ ra = a.aw1 + (size_t)k * D;
        const float* __restrict__ rc = a.cw1 + (size_t)k * D;
        for (int j = 0; j < D; ++j) {
            const float xj = xs[j];
            if constexpr (ACTOR) ha = fmaf(ra[j], xj, ha);
            if constexpr (CRITIC) hc = fmaf(rc[j], xj, hc);
        }
    }
    float* hrow = ps.h[slot][0];
    if constexpr (ACTOR) hrow[k] = tanhf(ha);
    if constexpr (CRITIC) hrow[kHidden + k] = tanhf(hc);
    PolicyFamily::sync();
    float ga = u0.z, gc = u0.w;
#pragma unroll 1
    for (int g = 0; g < kHidden / 4; ++g) {
        if constexpr (ACTOR) {
            const f4 w = ps.w2[0][g][k], hv = *(const f4*)(hrow + 4 * g);
            ga = fmaf(w.x, hv.x, ga); ga = fmaf(w.y, hv.y, ga); ga = fmaf(w.z, hv.z, ga); ga = fmaf(w.w, hv.w, ga);
        }
        if constexpr (CRITIC) {
            const f4 w = ps.w2[1][g][k], hv = *(const f4*)(hrow + kHidden + 4 * g);
            gc = fmaf(w.x, hv.x, gc); gc = fmaf(w.y, hv.y, gc); gc = fmaf(w.z, hv.z, gc); gc = fmaf(w.w, hv.w, gc);
        }
    }
    PolicyFamily::sync();       // (the next evaluation writes the activations again: in-order LDS, only the compiler is held)
    const f4 u1 = ps.unit[1][k];
    float p0 = 0.0f, p1 = 0.0f, pv = CRITIC ? u1.z * tanhf(gc) : 0.0f;
    if constexpr (ACTOR) {
        const float t = tanhf(ga);
        p0 = u1.x * t;
        p1 = u1.y * t;
    }
    wave_sum3(p0, p1, pv);
    m0 = p0;
    m1 = p1;
    v = pv;
}

// Box-Muller of Philox4x32-10 at counter (env, 0, total, kStreamPolicy): u1 in (0, 1], u2 in [0, 1)
__device__ __forceinline__ float2 policy_normal(const Params& p, uint32_t env_gid, uint32_t total) {
    const uint4 r = philox4x32_10(make_uint4(env_gid, 0u, total, kStreamPolicy), p.seed_lo, p.seed_hi);
    const float u1 = (float)((r.x >> 8) + 1u) * 0x1.0p-24f;
    const float u2 = (float)(r.y >> 8) * 0x1.0p-24f;
    const float rad = sqrtf(-2.0f * logf(u1));
    float s, c;
    sincospif(2.0f * u2, &s, &c);          // cos / sin(2 pi u2) with an exact argument (2 u2 is exact)
    return make_float2(rad * c, rad * s);
}

// The weights, the launch's arguments and the policy's constants into LDS, by the whole workgroup (before any wave may leave);
// the caller's __syncthreads() follows.  Shared by the policy rollout and the policy evaluation (evac_evaluate.h).
template <bool GRAV>
__device__ __forceinline__ void stage_policy(PolicySmem<GRAV>& ps, const PolicyArgs& ka, const NormArgs& kna) {
    for (int idx = (int)threadIdx.x; idx < 2 * (kHidden / 4) * kHidden; idx += PolicyFamily::kBlock) {
        const int m = idx / ((kHidden / 4) * kHidden), g = (idx / kHidden) % (kHidden / 4), k = idx % kHidden;
        const float* src = (m == 0 ? ka.aw2 : ka.cw2) + k * kHidden + 4 * g;
        ps.w2[m][g][k] = f4{src[0], src[1], src[2], src[3]};
    }
    for (int idx = (int)threadIdx.x; idx < 2 * kHidden; idx += PolicyFamily::kBlock) {
        const int m = idx / kHidden, k = idx % kHidden;
        ps.unit[m][k] = m == 0 ? f4{ka.ab1[k], ka.cb1[k], ka.ab2[k], ka.cb2[k]} : f4{ka.aw3[k], ka.aw3[kHidden + k], ka.cw3[k], 0.0f};
        if constexpr (GRAV) {
            const float* r = (m == 0 ? ka.aw1 : ka.cw1) + k * 6;
            ps.w1[m][0][k] = f4{r[0], r[1], r[2], r[3]};
            ps.w1[m][1][k] = f4{r[4], r[5], 0.0f, 0.0f};
        }
    }
    if (threadIdx.x == 0) {
        ps.args = ka;
        ps.na = kna;
        const float ls0 = ka.logstd[0], ls1 = ka.logstd[1], sd0 = expf(ls0), sd1 = expf(ls1);
        ps.c[0] = f4{ka.ab3[0], ka.ab3[1], ka.cb3[0], 0.0f};
        ps.c[1] = f4{sd0, sd1, sd0 * sd0, sd1 * sd1};
        ps.c[2] = f4{ls0, ls1, 0.0f, 0.0f};
    }
}

// An encoder between the observation and the actor-critic (ENC of the bodies below and of policy_evaluate_body): staged with
// the weights, run on the wave's observation row before every forward pass, and the actor-critic reads its row.  None here;
// evac_deepsets.h has one.
struct NoEncoder {
    static constexpr bool kOn = false;
};

// SHIFTED (the population form, k_collect_population): the wave's env is its place in the launch plus `env_shift`, and it has
// work while that is below `env_end` -- each learner's workgroups get the learner's own envs.
template <bool GRAV, bool NORM, bool SHIFTED = false, class ENC = NoEncoder>
__device__ __forceinline__ void policy_rollout_body(PolicyFamily::Smem& sm, PolicySmem<GRAV>& ps, const Params& p, int n_steps,
                                                    const PolicyArgs& ka, const NormArgs& kna, int env_shift = 0, int env_end = 0,
                                                    const ENC& enc = ENC{}) {
    using F = PolicyFamily;
    stage_policy<GRAV>(ps, ka, kna);
    if constexpr (ENC::kOn) enc.stage();
    __syncthreads();
    typename F::Ctx w(sm);
    if constexpr (SHIFTED) {
        w.env += env_shift;
        if (w.env >= env_end) return;
    } else {
        if (w.env >= p.n_envs) return;
    }
    F::init(w);
    const int k = w.lane, D = GRAV ? 6 : p.obs_dim, env = w.env;
    const bool active = w.i < p.n_ped;
    const size_t E = (size_t)p.n_envs;
    const PolicyArgs& a = ps.args;
    const NormArgs& na = ps.na;
    constexpr float kLogSqrt2Pi = 0.91893853320467274f;
    Ped q;
    Env e;
    load_env(p, env, w.i, active, q, e);
    const uint32_t gid = p.env_id_offset + (uint32_t)env;
    // the observation and done flag the call starts from: row 0 of the storage
    float* xs = ps.x[w.slot];
    for (int j = k; j < D; j += kWave) {
        const float v0 = a.next_obs[(size_t)env * D + j];
        xs[j] = v0;
        a.obs_out[(size_t)env * D + j] = v0;
    }
    float d = a.next_done[env];
    if (w.owner) a.done_out[env] = d;
    for (int t = 0; t < n_steps; ++t) {
        if ((t & 63) == 0) ps.z[w.slot][k] = policy_normal(p, gid, e.total + (uint32_t)k);   // the noise of the next 64 steps, one per lane
        F::sync();
        float m0, m1, v;
        if constexpr (ENC::kOn) {
            enc.encode(xs, w.slot, k, D, p.n_ped + 2);
            policy_eval<GRAV, true>(a, ps, w.slot, k, D, m0, m1, v, enc.row(w.slot));
        } else {
            policy_eval<GRAV, true>(a, ps, w.slot, k, D, m0, m1, v);
        }
        const f4 c0 = ps.c[0], c1 = ps.c[1], c2 = ps.c[2];
        m0 += c0.x;
        m1 += c0.y;
        v += c0.z;
        const float sd0 = c1.x, sd1 = c1.y, var0 = c1.z, var1 = c1.w, ls0 = c2.x, ls1 = c2.y;
        const float2 z = ps.z[w.slot][t & 63];
        const float z0 = z.x, z1 = z.y;
        const float a0 = m0 + sd0 * z0, a1 = m1 + sd1 * z1;
        const size_t te = (size_t)t * E + env;
        if (w.owner) {
            const float d0 = a0 - m0, d1 = a1 - m1;
            const float lp = (-(d0 * d0) / (2.0f * var0) - ls0 - kLogSqrt2Pi) + (-(d1 * d1) / (2.0f * var1) - ls1 - kLogSqrt2Pi);
            *(float2*)(a.actions_out + 2 * te) = make_float2(a0, a1);
            a.logprob_out[te] = lp;
            a.value_out[te] = v;
        }
        // the env step with this action: evac_step's kernel body (step_kernel_body) with the action from the policy
        float nz = 0.0f;
        if (ballot(needs_row(p, q.st)) != 0ull) nz = philox_noise(p, gid, w.i, e.total);
        StepOut o;
        step_env<F, GRAV>(p, w, active, q, e, agent_direction(p, a0, a1), nz, o);
        const bool done = o.terminated || o.truncated;
        double* ns = NORM ? na.state + (size_t)env * (3 * D + 4) : nullptr;
        float o6[6] = {e.ax, e.ay, o.ex, o.ey, o.gx, o.gy};
        if (done) {                          // wave-uniform, rare
            asm volatile("");
            if constexpr (NORM) {            // the terminal observation is counted first (SyncVectorEnv: the wrapped step, then reset)
                stage_observation<GRAV, F>(p, w, active, q, e, o6, xs);
#pragma unroll 1
                for (int j = k; j < D; j += kWave) {
                    double mean = ns[j], var = ns[D + j], cnt = ns[2 * D + j];
                    rms_update1(mean, var, cnt, (double)xs[j]);
                    ns[j] = mean; ns[D + j] = var; ns[2 * D + j] = cnt;
                }
                F::sync();
            }
            if (a.final_stats) {
                finish_counts<F>(p, w, q, o);
                if (w.owner) write_stats(a.final_stats + te, e, o);
            }
            reset_env(p, active, philox_reset_draw(p, gid, w.i, e.n_resets), q, e);
            F::invalidate(w);
            if constexpr (GRAV) grav_observation<F>(p, w, active, q, e, o6);
        }
        // the new observation (counted, normalised and clipped with NORM, as StoreNorm): row t + 1 of the storage, or next_obs
        // after the last step, and the wave's LDS row for the next step's policy
        stage_observation<GRAV, F>(p, w, active, q, e, o6, xs);
        float* dst = t + 1 < n_steps ? a.obs_out + ((size_t)(t + 1) * E + env) * D : a.next_obs + (size_t)env * D;
#pragma unroll 1
        for (int j = k; j < D; j += kWave) {
            float v = xs[j];
            if constexpr (NORM) {
                double mean = ns[j], var = ns[D + j], cnt = ns[2 * D + j];
                rms_update1(mean, var, cnt, (double)v);
                ns[j] = mean; ns[D + j] = var; ns[2 * D + j] = cnt;
                v = norm_clip((double)v, mean, var, (double)na.eps, na.obs_clip);
                xs[j] = v;
            }
            dst[j] = v;
        }
        d = done ? 1.0f : 0.0f;
        if (w.owner) {
            float r = o.reward;
            if constexpr (NORM) {   // gymnasium NormalizeReward, as step_outputs
                double mean = ns[3 * D], var = ns[3 * D + 1], cnt = ns[3 * D + 2], ret = ns[3 * D + 3];
                ret = ret * (double)na.gamma * (o.terminated ? 0.0 : 1.0) + (double)r;
                rms_update1(mean, var, cnt, ret);
                const double rv = (double)r / sqrt(var + (double)na.eps);
                r = clip_like_np(rv, na.reward_clip);
                ns[3 * D] = mean; ns[3 * D + 1] = var; ns[3 * D + 2] = cnt; ns[3 * D + 3] = ret;
            }
            a.reward_out[te] = r;
            if (t + 1 < n_steps) a.done_out[te + E] = d;
            else a.next_done[env] = d;
        }
    }
    F::sync();
    float m0, m1, v;
    if constexpr (ENC::kOn) {
        enc.encode(xs, w.slot, k, D, p.n_ped + 2);
        policy_eval<GRAV, false>(a, ps, w.slot, k, D, m0, m1, v, enc.row(w.slot));
    } else {
        policy_eval<GRAV, false>(a, ps, w.slot, k, D, m0, m1, v);   // the trainer's bootstrap get_value(next_obs)
    }
    if (w.owner) a.next_value_out[env] = v + ps.c[0].z;
    store_env(p, env, w.i, active, w.owner, q, e);
}

// DEF: the reference's default configuration as compile-time constants (default_config_constants; bit-identical)
template <bool GRAV, bool NORM, bool DEF>
__global__ __launch_bounds__(PolicyFamily::kBlock, 4) void k_policy_rollout(Params p, int n_steps, PolicyArgs a, NormArgs na) {
    __shared__ PolicyFamily::Smem sm;
    __shared__ PolicySmem<GRAV> ps;
    if constexpr (DEF) p = default_config_constants<GRAV>(p);
    policy_rollout_body<GRAV, NORM>(sm, ps, p, n_steps, a, na);
}

// ---- The population form: S learners' collection phases in one launch (include/evac.h: evac_policy_rollout_population) ----
// Learner s owns envs [s E_l, (s + 1) E_l) of the handle and `wgs` = ceil(E_l / 16) workgroups of the launch, so a workgroup
// never mixes learners: it stages learner s's 13 tensors (base + s x the tensor's stride) and runs policy_rollout_body on the
// learner's envs.  The waves past the learner's last env leave after the staging barrier, as the waves past the batch's end do.
struct PopulationArgs {
    int envs_per_learner, wgs;                  // E_l, ceil(E_l / 16)
    int64_t stride[13];                         // floats from learner s to learner s + 1, in evac_mlp_policy_t order
};
__device__ __forceinline__ PolicyArgs learner_policy(PolicyArgs a, const PopulationArgs& q, int s) {
    a.aw1 += s * q.stride[0]; a.ab1 += s * q.stride[1]; a.aw2 += s * q.stride[2]; a.ab2 += s * q.stride[3];
    a.aw3 += s * q.stride[4]; a.ab3 += s * q.stride[5]; a.logstd += s * q.stride[6];
    a.cw1 += s * q.stride[7]; a.cb1 += s * q.stride[8]; a.cw2 += s * q.stride[9]; a.cb2 += s * q.stride[10];
    a.cw3 += s * q.stride[11]; a.cb3 += s * q.stride[12];
    return a;
}
template <bool GRAV, bool NORM, bool DEF>
__global__ __launch_bounds__(PolicyFamily::kBlock, 4) void k_collect_population(Params p, int n_steps, PolicyArgs a, NormArgs na,
                                                                                PopulationArgs q) {
    __shared__ PolicyFamily::Smem sm;
    __shared__ PolicySmem<GRAV> ps;
    if constexpr (DEF) p = default_config_constants<GRAV>(p);
    const int s = (int)blockIdx.x / q.wgs;
    const PolicyArgs la = learner_policy(a, q, s);
    // (blockIdx.x x 16 + slot) + shift = s E_l + (blockIdx.x - s wgs) x 16 + slot
    policy_rollout_body<GRAV, NORM, true>(sm, ps, p, n_steps, la, na, s * (q.envs_per_learner - q.wgs * PolicyFamily::kEnvsPerBlock),
                                          (s + 1) * q.envs_per_learner);
}

// ---- ... with a NormalizeReward gamma per learner (include/evac.h: evac_policy_rollout_sweep) ----
// The reference wraps a learner's env with its training gamma, so in a gamma sweep every learner's chain has its own.  The
// values travel by value, indexed by the workgroup's learner (a scalar load from the kernel-argument segment); the body is
// k_collect_population's.  Only with the chain does gamma enter collection, hence NORM = true alone.
// TWIN: k_collect_sweep repeats k_collect_population's lines; change one, change the other.
struct LearnerGammas {
    float gamma[kMaxLearners];                  // (float)evac_learner_hyper_t.gamma of learner s
};
template <bool GRAV, bool DEF>
__global__ __launch_bounds__(PolicyFamily::kBlock, 4) void k_collect_sweep(Params p, int n_steps, PolicyArgs a, NormArgs na,
                                                                           PopulationArgs q, LearnerGammas lg) {
    __shared__ PolicyFamily::Smem sm;
    __shared__ PolicySmem<GRAV> ps;
    if constexpr (DEF) p = default_config_constants<GRAV>(p);
    const int s = (int)blockIdx.x / q.wgs;
    const PolicyArgs la = learner_policy(a, q, s);
    na.gamma = lg.gamma[s];
    policy_rollout_body<GRAV, true, true>(sm, ps, p, n_steps, la, na, s * (q.envs_per_learner - q.wgs * PolicyFamily::kEnvsPerBlock),
                                          (s + 1) * q.envs_per_learner);
}

}  // namespace evac
