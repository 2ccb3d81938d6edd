// What the entries that run a network on a handle's envs share (evac_api.hip: evac_policy_rollout*, evac_policy_evaluate*;
// evac_deepsets_api.hip, evac_transformer_api.hip: their forms with an encoder; evac_{deepsets,transformer}_population_api.hip: the
// collection of a population of such leaders; evac_{deepsets,transformer}_population_evaluate_api.hip: its evaluation;
// evac_capture_api.hip: the evaluation entries that record frames).  The handle's struct stays evac_api.hip's own:
// the handle_* functions are defined there and are not exported from the library.  Below them, host-only and inline: what
// every collection entry and every evaluation entry refuses, the one-wave limit, a population's shares of the envs, and the grid.
// Each returns the text that follows the entry's name in its message (empty: accepted), as mlp_policy_check does; the entry
// reports it through its own fail, at its own place in its order of checks.  Last, the whole bodies of the encoder entries as two
// templates over the unit's encoder (encoder_rollout, encoder_evaluate): those entries differ in nothing else.
#pragma once

#include <hip/hip_runtime.h>

#include <string>

#include "../../include/evac.h"
#include "evac_evaluate.h"
#include "evac_host.h"

namespace evac_host {

struct HandleView {
    evac::Params p;
    int device;
    bool default_cfg;       // the configuration the specialised (DEF) kernels assume
};

#define EVAC_HOST_LOCAL __attribute__((visibility("hidden")))
// What every entry with a handle checks first (a NULL handle, unbound state, a lost team): EVAC_OK and `out` filled, or the code
EVAC_HOST_LOCAL int handle_begin(evac_handle_t h, const char* what, HandleView* out);
// Handles with parts = 2 or chain = 1 / 2 are joined: `stream` waits for their own streams
EVAC_HOST_LOCAL int handle_settle(evac_handle_t h, hipStream_t stream);
// `msg` becomes evac_last_error(h); returns `code`
EVAC_HOST_LOCAL int handle_fail(evac_handle_t h, int code, const std::string& msg);
EVAC_HOST_LOCAL int handle_check_launch(evac_handle_t h, const char* what);
// The scripted agent's turning points for this handle's room (EvalArgs::thr_x, thr_y)
EVAC_HOST_LOCAL void handle_turning_points(evac_handle_t h, float* thr_x, float* thr_y);
#undef EVAC_HOST_LOCAL

}  // namespace evac_host

namespace {

// One wave per env (EVAC_ERR_UNSUPPORTED): the collection entries refuse it first, the evaluation entries last.
inline std::string one_wave_check(const evac::Params& p) {
    if (p.n_ped > evac::kWave) return ": rooms of more than 64 pedestrians are not supported (one wave per env)";
    return {};
}
// One workgroup per kEnvsPerBlock envs (of the handle, or of a learner's share).
inline int policy_wgs(int n_envs) { return (n_envs + evac::PolicyFamily::kEnvsPerBlock - 1) / evac::PolicyFamily::kEnvsPerBlock; }

// The outputs of a collection launch; the 13 pointers in front of them are mlp_policy_check's.
inline evac::PolicyArgs collect_outputs(float* next_obs, float* next_done, float* obs_out, float* actions_out, float* logprob_out,
                                        float* value_out, float* reward_out, float* done_out, float* next_value_out,
                                        evac_episode_stats_t* final_stats) {
    evac::PolicyArgs a{};
    a.next_obs = next_obs; a.next_done = next_done; a.obs_out = obs_out; a.actions_out = actions_out; a.logprob_out = logprob_out;
    a.value_out = value_out; a.reward_out = reward_out; a.done_out = done_out; a.next_value_out = next_value_out;
    a.final_stats = final_stats;
    return a;
}
// What every collection entry refuses of its step count and buffers (`a`: collect_outputs), before it looks at the networks.
// `policy_named`: the linear entries refuse a NULL policy with the same message, the encoder entries with their networks.
inline std::string collect_check(int32_t n_steps, const evac::PolicyArgs& a, bool policy_named, const evac_mlp_policy_t* policy) {
    if (n_steps < 1) return ": n_steps must be >= 1";
    const bool buffers = a.next_obs && a.next_done && a.obs_out && a.actions_out && a.logprob_out && a.value_out && a.reward_out &&
                         a.done_out && a.next_value_out;
    if (!buffers || (policy_named && !policy))
        return std::string(policy_named ? ": policy and every" : ": every") + " output buffer but final_stats / norm_state must be non-NULL";
    return {};
}
// ... and after the networks (the kernels store an action as one float2)
inline std::string collect_aligned(const evac::PolicyArgs& a) {
    if ((uintptr_t)a.actions_out & 7u) return ": actions_out must be 8-byte aligned";
    return {};
}

// What every evaluation entry refuses of its counts and buffers, after the agent code and before the networks, and the
// arguments it launches with (the scripted agent's turning points left 0).
inline std::string evaluate_check(int32_t agent, int32_t n_episodes, int32_t max_steps, int32_t* progress, evac_episode_stats_t* episodes_out,
                                  const double* norm_state, float obs_clip, float epsilon, evac::EvalArgs& ev) {
    if (!progress || !episodes_out) return ": progress / episodes_out is NULL";
    if (n_episodes < 1 || max_steps < 1) return ": n_episodes and max_steps must be >= 1";
    if (agent == EVAC_AGENT_VACUUM_CLEANER && norm_state) return ": the scripted agent reads no observation: norm_state must be NULL";
    if ((uintptr_t)progress & 15u) return ": progress must be 16-byte aligned";
    ev = evac::EvalArgs{(int4*)progress, episodes_out, norm_state, (int)n_episodes, (int)max_steps,
                        agent == EVAC_AGENT_POLICY_SAMPLE ? 1 : 0, obs_clip, epsilon, 0.0f, 0.0f};
    return {};
}

// What a recording evaluation entry refuses of its capture, after its counterpart's own checks, and the arguments its kernel takes.
inline std::string capture_check(const evac_eval_capture_t* c, int n_envs, evac::EvalCaptureArgs& ca) {
    if (!c) return ": capture is NULL";
    if (c->capture_envs < 1 || c->capture_envs > n_envs) return ": capture_envs must be in 1.." + std::to_string(n_envs);
    if (c->max_frames < 1) return ": max_frames must be >= 1";
    if (!c->frames || !c->starts) return ": frames / starts is NULL";
    ca = evac::EvalCaptureArgs{c->frames, c->starts, (int)c->capture_envs, (int)c->max_frames};
    return {};
}

// A population's equal shares of a handle's envs into `q`: the learners' number, the envs divisible by it, every stride at least
// its tensor.
inline std::string learner_shares(int n_envs, int32_t n_learners, const evac_mlp_policy_strides_t* strides, int32_t obs_dim,
                                  evac::PopulationArgs& q) {
    if (n_learners < 1 || n_learners > EVAC_MAX_LEARNERS) return ": n_learners must be in 1.." + std::to_string(EVAC_MAX_LEARNERS);
    if (n_envs % n_learners != 0)
        return ": the handle's " + std::to_string(n_envs) + " envs are not " + std::to_string(n_learners) + " learners' equal shares";
    if (!mlp_strides_ok(strides, obs_dim, n_learners, q.stride)) return ": a learner stride is smaller than its tensor";
    q.envs_per_learner = n_envs / n_learners;
    q.wgs = policy_wgs(q.envs_per_learner);
    return {};
}

// The entries of a network with an encoder in front of the actor-critic (evac_deepsets_api.hip, evac_transformer_api.hip), over
// the unit's trait Enc:
//   Struct, Args                     the encoder as include/evac.h has it and as the kernels take it
//   kRollout, kEvaluate              the entries' names
//   check(p, S, args, why)           the encoder against the handle, after the policy's own check: EVAC_OK and `args` filled, or
//                                    the code with the text that follows the entry's name in `why`
//   rollout_kernel(norm, def), evaluate_kernel(norm, def)      the instantiations of the unit's two kernel templates
// and, in the unit of the recording evaluation (evac_capture_api.hip) alone: kCapture, capture_kernel(norm).
// What both entries refuse of the two networks, in this order: no policy, no encoder, the thirteen tensors (into `a`), Enc's own.
template <class Enc>
inline int encoder_networks_check(const evac::Params& p, const evac_mlp_policy_t* policy, const typename Enc::Struct* encoder,
                                  evac::PolicyArgs& a, typename Enc::Args& ea, std::string& why) {
    if (!policy) return why = ": policy is NULL", EVAC_ERR_INVALID_ARGUMENT;
    if (!encoder) return why = ": encoder is NULL", EVAC_ERR_INVALID_ARGUMENT;
    if (!(why = mlp_policy_check(*policy, p.obs_dim, a)).empty()) return EVAC_ERR_INVALID_ARGUMENT;
    return Enc::check(p, *encoder, ea, why);
}

// A lone learner: nothing more to refuse, the whole handle in Enc's own kernel.
struct NoLearners {
    static constexpr bool kOn = false;
};
// What a population form refuses first behind the handle: its Learners' `strides` / `enc_strides` (the two C structs) missing.
constexpr const char* kNullStrides = ": strides / enc_strides is NULL";
// evac_policy_rollout_<encoder> (`a`: collect_outputs).  Every refusal before the first HIP call; one kernel on `stream`.
// Learners (kOn): the population form of the entry (evac_{deepsets,transformer}_population_api.hip) -- a NULL `strides` /
// `enc_strides` of it is refused first behind the handle, check(p, policy, encoder) adds its refusals behind the networks' and
// before the alignment of actions_out, in the same form, and launch(view, n_steps, a, na, ea, stream) enqueues its own kernel.
template <class Enc, class Learners = NoLearners>
inline int encoder_rollout(evac_handle_t h, int32_t n_steps, const evac_mlp_policy_t* policy, evac::PolicyArgs a, const evac::NormArgs& na,
                           const typename Enc::Struct* encoder, void* stream, Learners learners = Learners{}) {
    using evac_host::handle_fail;
    const std::string w = Enc::kRollout;
    evac_host::HandleView v;
    if (const int rc = evac_host::handle_begin(h, w.c_str(), &v); rc != EVAC_OK) return rc;
    if constexpr (Learners::kOn) {
        if (!learners.strides || !learners.enc_strides) return handle_fail(h, EVAC_ERR_INVALID_ARGUMENT, w + kNullStrides);
    }
    std::string why = one_wave_check(v.p);
    if (!why.empty()) return handle_fail(h, EVAC_ERR_UNSUPPORTED, w + why);
    typename Enc::Args ea{};
    why = collect_check(n_steps, a, false, policy);    // (the first refusal in the entry's order of checks)
    if (!why.empty()) return handle_fail(h, EVAC_ERR_INVALID_ARGUMENT, w + why);
    if (const int rc = encoder_networks_check<Enc>(v.p, policy, encoder, a, ea, why); rc != EVAC_OK) return handle_fail(h, rc, w + why);
    if constexpr (Learners::kOn) {
        if (!(why = learners.check(v.p, *policy, *encoder)).empty()) return handle_fail(h, EVAC_ERR_INVALID_ARGUMENT, w + why);
    }
    why = collect_aligned(a);
    if (!why.empty()) return handle_fail(h, EVAC_ERR_INVALID_ARGUMENT, w + why);
    if (const int st = evac_host::handle_settle(h, (hipStream_t)stream); st != EVAC_OK) return st;
    DeviceGuard g(v.device);
    if constexpr (Learners::kOn) {
        learners.launch(v, (int)n_steps, a, na, ea, (hipStream_t)stream);
    } else {
        hipLaunchKernelGGL(Enc::rollout_kernel(na.state != nullptr, v.default_cfg), dim3((unsigned)policy_wgs(v.p.n_envs)),
                           dim3(evac::PolicyFamily::kBlock), 0, (hipStream_t)stream, v.p, (int)n_steps, a, na, ea);
    }
    return evac_host::handle_check_launch(h, w.c_str());
}

// evac_policy_evaluate_<encoder>: the agent's code first, the one-wave limit last.  CAPTURE: evac_policy_evaluate_<encoder>_capture,
// the same with capture_check behind the one-wave limit and the capture behind the kernel's arguments.
// Learners (kOn): the population form of the entry (evac_{deepsets,transformer}_population_evaluate_api.hip;
// Enc::kEvaluatePopulation its name) -- a NULL `strides` / `enc_strides` of it is refused first behind the handle,
// check(p, policy, encoder) adds its refusals behind the networks' and before the one-wave limit, and
// launch(view, a, ev, ea, stream) enqueues its own kernel.
template <class Enc, bool CAPTURE = false, class Learners = NoLearners>
inline int encoder_evaluate(evac_handle_t h, int32_t agent, const evac_mlp_policy_t* policy, int32_t n_episodes, int32_t max_steps,
                            int32_t* progress, evac_episode_stats_t* episodes_out, const double* norm_state, float obs_clip, float epsilon,
                            const typename Enc::Struct* encoder, void* stream, const evac_eval_capture_t* capture = nullptr,
                            Learners learners = Learners{}) {
    static_assert(!(CAPTURE && Learners::kOn), "recording is one network's");
    using evac_host::handle_fail;
    std::string w;
    if constexpr (CAPTURE) w = Enc::kCapture;
    else if constexpr (Learners::kOn) w = Enc::kEvaluatePopulation;
    else w = Enc::kEvaluate;
    evac_host::HandleView v;
    if (const int rc = evac_host::handle_begin(h, w.c_str(), &v); rc != EVAC_OK) return rc;
    if constexpr (Learners::kOn) {
        if (!learners.strides || !learners.enc_strides) return handle_fail(h, EVAC_ERR_INVALID_ARGUMENT, w + kNullStrides);
    }
    if (agent == EVAC_AGENT_VACUUM_CLEANER)
        return handle_fail(h, EVAC_ERR_INVALID_ARGUMENT, w + ": the scripted agent has no network (use evac_policy_evaluate)");
    if (agent != EVAC_AGENT_POLICY_MEAN && agent != EVAC_AGENT_POLICY_SAMPLE)
        return handle_fail(h, EVAC_ERR_INVALID_ARGUMENT, w + ": unknown agent " + std::to_string(agent));
    evac::EvalArgs ev{};
    evac::PolicyArgs a{};
    typename Enc::Args ea{};
    std::string why = evaluate_check(agent, n_episodes, max_steps, progress, episodes_out, norm_state, obs_clip, epsilon, ev);
    if (!why.empty()) return handle_fail(h, EVAC_ERR_INVALID_ARGUMENT, w + why);
    if (const int rc = encoder_networks_check<Enc>(v.p, policy, encoder, a, ea, why); rc != EVAC_OK) return handle_fail(h, rc, w + why);
    if constexpr (Learners::kOn) {
        if (!(why = learners.check(v.p, *policy, *encoder)).empty()) return handle_fail(h, EVAC_ERR_INVALID_ARGUMENT, w + why);
    }
    if (!(why = one_wave_check(v.p)).empty()) return handle_fail(h, EVAC_ERR_UNSUPPORTED, w + why);
    evac::EvalCaptureArgs ca{};
    if constexpr (CAPTURE) {
        if (!(why = capture_check(capture, v.p.n_envs, ca)).empty()) return handle_fail(h, EVAC_ERR_INVALID_ARGUMENT, w + why);
    }
    if (const int st = evac_host::handle_settle(h, (hipStream_t)stream); st != EVAC_OK) return st;
    DeviceGuard g(v.device);
    const dim3 grid((unsigned)policy_wgs(v.p.n_envs)), block(evac::PolicyFamily::kBlock);
    if constexpr (CAPTURE) {
        hipLaunchKernelGGL(Enc::capture_kernel(norm_state != nullptr), grid, block, 0, (hipStream_t)stream, v.p, a, ev, ea, ca);
    } else if constexpr (Learners::kOn) {
        learners.launch(v, a, ev, ea, (hipStream_t)stream);
    } else {
        hipLaunchKernelGGL(Enc::evaluate_kernel(norm_state != nullptr, v.default_cfg), grid, block, 0, (hipStream_t)stream, v.p, a, ev, ea);
    }
    return evac_host::handle_check_launch(h, w.c_str());
}

}  // namespace
