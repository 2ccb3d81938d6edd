// Device code of libevac, part 6: the POLICY EVALUATION -- whole episodes per env under a FIXED agent, one episode record per
// finished episode and nothing else (no storage rows, no values, no statistics update).  The reference has no such loop of its
// own: it is what a user writes around a trained RPOLinearNetwork (rpo_linear_agent_network.py:49-61 with the mean as the action)
// or around the scripted baseline (baseline_wacuum_cleaner.py) and EvacuationEnv.step / reset (env.py:106-171).
//
// Geometry, step body, reset, episode records and the Philox streams are the policy rollout's (evac_policy.h): one wave per env
// (N <= 64), 16 envs per workgroup, the weights staged once per workgroup by stage_policy, the forward pass by policy_eval (the
// actor alone: CRITIC = false), the sampled action from policy_normal at the rollout's own counter.  The env side is
// step_env / finish_counts / write_stats / reset_env exactly as evac_step runs them, so an evaluation in sample mode is the
// policy rollout bit for bit, and one in mean mode is the policy rollout with sigma = 0.
//
// An env runs until it has finished n_episodes episodes or max_steps steps of this launch, whichever comes first, and stores its
// state and its progress words back: the next launch continues where this one stopped, bit for bit.  Every loop is bounded by
// max_steps.  A wave whose env is done leaves; its workgroup lasts as long as its longest env.
#pragma once

#include "evac_policy.h"

namespace evac {

struct EvalArgs {
    int4* progress;                       // [E] {episodes finished, steps taken, two words of the scripted agent's state}: in / out
    evac_episode_stats_t* episodes_out;   // [n_episodes][E]
    const double* norm_state;             // [E][3 D + 4] or NULL: the trainer's observation statistics, READ ONLY (frozen)
    int n_episodes, max_steps;
    int sample;                           // policy agents: 0 the mean, 1 mean + sigma z
    float obs_clip, eps;
    float thr_x, thr_y;                   // scripted agent: the sweep's turning points (see vacuum_action)
};

struct EvalSmem {
    EvalArgs a;                                    // the launch's arguments, read back where they are used (as PolicySmem::args)
    int n_done[PolicyFamily::kEnvsPerBlock];       // episodes finished, per env of the workgroup
};

// Recording for rendering (include/evac.h: evac_eval_capture_t): the frames of envs 0 .. capture_envs - 1, in capture_state's
// layout (evac_device.h).  frames[f] is the state after the env's step f, counted from the env's first step of the evaluation and
// before any reset (Pedestrians.save / Agent.save in step); starts[k] is the state episode k begins with (Pedestrians.save in reset).
struct EvalCaptureArgs {
    float* frames;                        // [max_frames][capture_envs][N + 1][3]
    float* starts;                        // [n_episodes][capture_envs][N + 1][3]
    int capture_envs, max_frames;
};

struct EvalCaptureSmem {
    EvalCaptureArgs a;                             // (read back where used, as EvalSmem::a)
    // per env of the workgroup, set when the launch begins: where the frame of its step 0 of this launch goes (the env's own
    // column of frames: the row of step t is t rows of all K envs further on), how many steps of this launch still have a row
    // (0: the env is not recorded, or is past max_frames), and the env's column of starts (NULL: not recorded)
    struct Env {
        float* first;
        float* start;
        int rows;
    } env[PolicyFamily::kEnvsPerBlock];
};

// The capture policy of policy_evaluate_body: none (the default; no code) ...
struct NoCapture {
    static constexpr bool kOn = false;
};
// ... or the frames above.  Arguments and the env's place in the frames live in LDS, as EvalSmem's n_done does: the step takes
// every register, so a step reads back a pointer and a count and forms the row's address in scalar registers.
struct EvalCapture {
    static constexpr bool kOn = true;
    EvalCaptureSmem& cs;
    const EvalCaptureArgs& ka;

    // by the whole workgroup, before the staging barrier (beside es.a)
    __device__ __forceinline__ void stage() const {
        if (threadIdx.x == 0) cs.a = ka;
    }
    // the wave's env starts this launch after `steps` steps of the evaluation
    __device__ __forceinline__ void begin(const Params& p, const PolicyFamily::Ctx& w, int steps) const {
        if (w.owner) {
            const EvalCaptureArgs& a = cs.a;
            const bool recorded = w.env < a.capture_envs;
            cs.env[w.slot].first = a.frames + (((size_t)steps * a.capture_envs + w.env) * (p.n_ped + 1)) * 3;
            cs.env[w.slot].start = recorded ? a.starts + ((size_t)w.env * (p.n_ped + 1)) * 3 : nullptr;
            cs.env[w.slot].rows = recorded && steps < a.max_frames ? a.max_frames - steps : 0;
        }
        PolicyFamily::sync();
    }
    // At the top of every step: the lane's indices pass through an empty asm, so what is derived from them (LDS addresses, row
    // offsets) is formed again inside the step and not kept in vector registers across it.  Those are the registers the
    // capture's stores take: without this the encoder kernels with a normaliser spill.  The values do not change.
    __device__ __forceinline__ void relieve(PolicyFamily::Ctx& w) const { asm volatile("" : "+v"(w.lane), "+v"(w.i)); }
    // What LDS gives back is the same in every lane of the wave: read into scalar registers
    static __device__ __forceinline__ int uni(int v) { return __builtin_amdgcn_readfirstlane(v); }
    static __device__ __forceinline__ float* uni(float* ptr) {
        const unsigned long long u = (unsigned long long)ptr;
        return (float*)(((unsigned long long)(unsigned)uni((int)(u >> 32)) << 32) | (unsigned)uni((int)u));
    }
    // the state episode k < n_episodes begins with
    __device__ __forceinline__ void start(const Params& p, const PolicyFamily::Ctx& w, bool active, const Ped& q, const Env& e, int k) const {
        float* const col = uni(cs.env[w.slot].start);
        if (col) capture_state(p, col, uni(cs.a.capture_envs), uni(k), 0, w.i, active, w.owner, q, e);     // (env 0: as in step)
    }
    // the state after step t of this launch, before any reset
    __device__ __forceinline__ void step(const Params& p, const PolicyFamily::Ctx& w, bool active, const Ped& q, const Env& e, int t) const {
        const EvalCaptureSmem::Env& c = cs.env[w.slot];
        if (uni(t) >= uni(c.rows)) return;
        // (`first` is the env's own column: env 0 of the K that capture_state strides over)
        capture_state(p, uni(c.first), uni(cs.a.capture_envs), uni(t), 0, w.i, active, w.owner, q, e);
    }
};

// The reference's sweep baseline (baseline_wacuum_cleaner.py:7-82) as a state machine over the leader's position alone:
//   climb   until y >= thr_y (then one step right, and sweep)
//   sweep   right until x >= thr_x, or left until x <= -thr_x; at a turn: one step down, the direction flips and the next 25 steps
//           go down as long as y > -thr_y -- the first of them that finds y <= -thr_y ends the sweep
//   exit    the action is exit - position
// thr = extent - SWITCH_DISTANCE_TO_LEADER / 2 + step_size, formed in double on the host and rounded once: the reference compares a
// float32 position with that Python float, which NumPy 2 does in float32.  s0 = phase | direction << 2 (0 right, 1 left),
// s1 = the countdown; all zero = a fresh agent.
__device__ __forceinline__ float2 vacuum_action(float x, float y, float thr_x, float thr_y, int& s0, int& s1) {
    int phase = s0 & 3, left = (s0 >> 2) & 1;
    float2 a = make_float2(kExitX - x, kExitY - y);
    if (phase == 0) {
        if (y < thr_y) {
            a = make_float2(0.0f, 1.0f);
        } else {
            phase = 1;
            a = make_float2(1.0f, 0.0f);
        }
    } else if (phase == 1) {
        if (s1 > 0) {
            s1 -= 1;
            if (y > -thr_y) a = make_float2(0.0f, -1.0f);
            else phase = 2;
        } else if (left ? x > -thr_x : x < thr_x) {
            a = make_float2(left ? -1.0f : 1.0f, 0.0f);
        } else {
            left ^= 1;
            s1 = 25;
            a = make_float2(0.0f, -1.0f);
        }
    }
    s0 = phase | (left << 2);
    return a;
}

// The observation the policy reads, from the CURRENT state, into the wave's LDS row: the raw observation (stage_observation),
// then -- NORM -- norm_clip with the env's own row of norm_state, which is only read.
template <bool GRAV, bool NORM>
__device__ __forceinline__ void eval_observation(const Params& p, PolicyFamily::Ctx& w, bool active, const Ped& q, const Env& e,
                                                 const float (&o6)[6], float* xs, const EvalArgs& ev, int D) {
    if constexpr (GRAV && NORM) {        // six features: lane j owns feature j (stage_observation's selection) and normalises it
        if (w.lane < 6) {
            float v = o6[0];
#pragma unroll
            for (int j = 1; j < 6; ++j) v = w.lane == j ? o6[j] : v;
            const double* ns = ev.norm_state + (size_t)w.env * (3 * 6 + 4) + w.lane;
            xs[w.lane] = norm_clip((double)v, ns[0], ns[6], (double)ev.eps, ev.obs_clip);
        }
        PolicyFamily::sync();
    } else {
        stage_observation<GRAV, PolicyFamily>(p, w, active, q, e, o6, xs);
        if constexpr (NORM) {
            const double* ns = ev.norm_state + (size_t)w.env * (3 * D + 4);
#pragma unroll 1
            for (int j = w.lane; j < D; j += kWave) xs[j] = norm_clip((double)xs[j], ns[j], ns[D + j], (double)ev.eps, ev.obs_clip);
            PolicyFamily::sync();
        }
    }
}

// POLICY: the network is the agent (ps: its weights in LDS); else the scripted baseline, which reads e.ax / e.ay and nothing else.
// ENC: an encoder in front of the actor (evac_policy.h: NoEncoder; evac_deepsets.h).
// SHIFTED (the population form, k_evaluate_population): as policy_rollout_body's -- the wave's env is its place in the launch plus
// `env_shift`, and it has work while that is below `env_end`; the env's global id, which keys every Philox stream of the body, is
// further back by `id_shift` (a learner's share with the ids of learner 0's: the same episodes for every learner).
// CAP: the capture policy (NoCapture; EvalCapture, evac_capture_api.hip's kernels).  A launch sequence writes the frames of one long
// launch: the row comes from the progress word and nothing new is carried.
template <bool POLICY, bool GRAV, bool NORM, class ENC = NoEncoder, bool SHIFTED = false, class CAP = NoCapture>
__device__ __forceinline__ void policy_evaluate_body(PolicyFamily::Smem& sm, PolicySmem<GRAV>* psp, EvalSmem& es, const Params& p,
                                                     const PolicyArgs& ka, const EvalArgs& kev, const ENC& enc = ENC{},
                                                     int env_shift = 0, int env_end = 0, int id_shift = 0, const CAP& cap = CAP{}) {
    using F = PolicyFamily;
    if constexpr (POLICY) stage_policy<GRAV>(*psp, ka, NormArgs{nullptr, 0.f, 0.f, 0.f, 0.f});
    if constexpr (ENC::kOn) enc.stage();
    if constexpr (CAP::kOn) cap.stage();
    if (threadIdx.x == 0) es.a = kev;
    __syncthreads();
    typename F::Ctx w(sm);
    if constexpr (SHIFTED) {
        w.env += env_shift;
        if (w.env >= env_end) return;
    } else {
        if (w.env >= p.n_envs) return;
    }
    const EvalArgs& ev = es.a;
    const int env = w.env;
    // The env's progress words stay out of the registers (the step takes them all, as in policy_rollout_body): the episode count
    // lives in LDS and changes in the rare branch alone, the step count is the loop's own counter, and the scripted agent's two
    // words are live in its kernels only.
    const int4 pr = ev.progress[env];
    // this env has finished: nothing is read or written (a negative count -- not a progress word of this library -- would index
    // in front of episodes_out: such an env is left alone too)
    if (pr.x < 0 || pr.x >= ev.n_episodes) return;
    if (w.owner) es.n_done[w.slot] = pr.x;
    int s0 = 0, s1 = 0;
    if constexpr (!POLICY) {
        s0 = __builtin_amdgcn_readfirstlane(pr.z);
        s1 = __builtin_amdgcn_readfirstlane(pr.w);
    }
    F::init(w);
    const int k = w.lane, D = GRAV ? 6 : p.obs_dim;
    const bool active = w.i < p.n_ped;
    Ped q;
    Env e;
    load_env(p, env, w.i, active, q, e);
    if constexpr (CAP::kOn) {
        cap.begin(p, w, pr.y);
        if (pr.x == 0 && pr.y == 0) cap.start(p, w, active, q, e, 0);       // the evaluation's first launch for this env
    }
    uint32_t gid = p.env_id_offset + (uint32_t)env;
    if constexpr (SHIFTED) gid = p.env_id_offset + (uint32_t)(env - id_shift);
    float* xs = nullptr;
    float o6[6] = {};
    if constexpr (POLICY) xs = psp->x[w.slot];
    bool fresh = true;                             // no step of this launch has left the gravity observation of the state: the
                                                   // launch's start and every reset take it by a full reduction
    int t = 0;                                     // steps of this launch
    while (t < ev.max_steps) {
        if constexpr (CAP::kOn) cap.relieve(w);
        float a0, a1;
        if constexpr (POLICY) {
            PolicySmem<GRAV>& ps = *psp;
            if constexpr (GRAV) {
                if (fresh) {                       // wave-uniform, rare
                    asm volatile("");
                    grav_observation<F>(p, w, active, q, e, o6);
                }
            }
            eval_observation<GRAV, NORM>(p, w, active, q, e, o6, xs, ev, D);
            const bool sample = ev.sample != 0;
            if (sample && (t & 63) == 0) ps.z[w.slot][k] = policy_normal(p, gid, e.total + (uint32_t)k);   // as policy_rollout_body
            F::sync();
            float m0, m1, v;
            if constexpr (ENC::kOn) {
                enc.encode(xs, w.slot, k, D, p.n_ped + 2);
                policy_eval<GRAV, true, false>(ps.args, ps, w.slot, k, D, m0, m1, v, enc.row(w.slot));
            } else {
                policy_eval<GRAV, true, false>(ps.args, ps, w.slot, k, D, m0, m1, v);
            }
            const f4 c0 = ps.c[0];
            m0 += c0.x;
            m1 += c0.y;
            a0 = m0;
            a1 = m1;
            if (sample) {
                const f4 c1 = ps.c[1];
                const float2 z = ps.z[w.slot][t & 63];
                a0 = m0 + c1.x * z.x;
                a1 = m1 + c1.y * z.y;
            }
        } else {
            const float2 a = vacuum_action(e.ax, e.ay, ev.thr_x, ev.thr_y, s0, s1);
            a0 = a.x;
            a1 = a.y;
        }
        // the env step with this action: evac_step's kernel body (step_kernel_body)
        float nz = 0.0f;
        if (ballot(needs_row(p, q.st)) != 0ull) nz = philox_noise(p, gid, w.i, e.total);
        StepOut o;
        step_env<F, GRAV>(p, w, active, q, e, agent_direction(p, a0, a1), nz, o);
        if constexpr (CAP::kOn) cap.step(p, w, active, q, e, t);
        t += 1;
        o6[0] = e.ax; o6[1] = e.ay; o6[2] = o.ex; o6[3] = o.ey; o6[4] = o.gx; o6[5] = o.gy;
        fresh = false;
        if (o.terminated || o.truncated) {       // wave-uniform, rare
            asm volatile("");
            F::sync();
            const int n_done = __builtin_amdgcn_readfirstlane(es.n_done[w.slot]);
            finish_counts<F>(p, w, q, o);
            if (w.owner) {
                write_stats(ev.episodes_out + (size_t)n_done * (size_t)p.n_envs + env, e, o);
                es.n_done[w.slot] = n_done + 1;
            }
            s0 = s1 = 0;                         // a scripted agent starts afresh with every episode
            reset_env(p, active, philox_reset_draw(p, gid, w.i, e.n_resets), q, e);
            if constexpr (CAP::kOn) {
                if (n_done + 1 < ev.n_episodes) cap.start(p, w, active, q, e, n_done + 1);
            }
            F::invalidate(w);
            fresh = true;
            if (n_done + 1 >= ev.n_episodes) break;
        }
    }
    store_env(p, env, w.i, active, w.owner, q, e);
    if (w.owner) {
        int* pw = (int*)(ev.progress + env);
        pw[0] = es.n_done[w.slot];
        pw[1] += t;
        if constexpr (!POLICY) {
            pw[2] = s0;
            pw[3] = s1;
        }
    }
}

// DEF: the reference's default configuration as compile-time constants (default_config_constants; bit-identical)
template <bool GRAV, bool NORM, bool DEF>
__global__ __launch_bounds__(PolicyFamily::kBlock, 4) void k_policy_evaluate(Params p, PolicyArgs a, EvalArgs ev) {
    __shared__ PolicyFamily::Smem sm;
    __shared__ PolicySmem<GRAV> ps;
    __shared__ EvalSmem es;
    if constexpr (DEF) p = default_config_constants<GRAV>(p);
    policy_evaluate_body<true, GRAV, NORM>(sm, &ps, es, p, a, ev);
}

// The scripted baseline: no weights, no observation, no normaliser -- the step body without the observation's sums
template <bool DEF>
__global__ __launch_bounds__(PolicyFamily::kBlock, 4) void k_policy_evaluate_scripted(Params p, EvalArgs ev) {
    __shared__ PolicyFamily::Smem sm;
    __shared__ EvalSmem es;
    if constexpr (DEF) p = default_config_constants<false>(p);
    policy_evaluate_body<false, false, false>(sm, (PolicySmem<false>*)nullptr, es, p, PolicyArgs{}, ev);
}

// ---- The population form: S learners' evaluations in one launch (include/evac.h: evac_policy_evaluate_population) ----
// k_collect_population's geometry (evac_policy.h): learner s owns envs [s E_l, (s + 1) E_l) of the handle and `wgs` workgroups of
// the launch, stages its own 13 tensors and runs policy_evaluate_body on its envs.  progress, episodes_out and norm_state are
// indexed by the handle's env.  shared != 0: learner s's env i draws with the id of env i, whoever the learner is.
template <bool GRAV, bool NORM, bool DEF>
__global__ __launch_bounds__(PolicyFamily::kBlock, 4) void k_evaluate_population(Params p, PolicyArgs a, EvalArgs ev, PopulationArgs q,
                                                                                 int shared) {
    __shared__ PolicyFamily::Smem sm;
    __shared__ PolicySmem<GRAV> ps;
    __shared__ EvalSmem es;
    if constexpr (DEF) p = default_config_constants<GRAV>(p);
    const int s = (int)blockIdx.x / q.wgs;
    const PolicyArgs la = learner_policy(a, q, s);
    // (blockIdx.x x 16 + slot) + shift = s E_l + (blockIdx.x - s wgs) x 16 + slot
    policy_evaluate_body<true, GRAV, NORM, NoEncoder, true>(sm, &ps, es, p, la, ev, NoEncoder{},
                                                            s * (q.envs_per_learner - q.wgs * PolicyFamily::kEnvsPerBlock),
                                                            (s + 1) * q.envs_per_learner, shared ? s * q.envs_per_learner : 0);
}

}  // namespace evac
