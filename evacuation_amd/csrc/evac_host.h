// Host-only helpers shared by the six translation units of libevac: which device a call runs on; the 13 tensors of the
// actor-critic as an array, their sizes, the check of a population's strides and of a policy against a handle; the picker of a
// kernel template's instantiation over bools; what every entry refuses of evac_learner_hyper_t.
#pragma once

#include <hip/hip_runtime.h>
#include <stddef.h>

#include <string>

#include "../../include/evac.h"

namespace {

struct DeviceGuard {
    int prev = -1;
    bool switched = false;
    explicit DeviceGuard(int dev) {
        if (dev >= 0 && hipGetDevice(&prev) == hipSuccess && prev != dev) switched = hipSetDevice(dev) == hipSuccess;
    }
    ~DeviceGuard() {
        if (switched) (void)hipSetDevice(prev);
    }
};

// The device that owns `p`, or -1: for the entries without a handle (the kernels must run on the device that owns the buffers).
inline int device_of(const void* p) {
    hipPointerAttribute_t attr;
    if (hipPointerGetAttributes(&attr, p) == hipSuccess) return attr.device;
    (void)hipGetLastError();
    return -1;
}

// evac_mlp_policy_t (from actor_w1 on) and evac_mlp_policy_grads_t are 13 consecutive float pointers in the same order.
constexpr int kMlpTensors = 13;
static_assert(sizeof(evac_mlp_policy_grads_t) == kMlpTensors * sizeof(float*) &&
                  offsetof(evac_mlp_policy_grads_t, critic_b3) == (kMlpTensors - 1) * sizeof(float*) &&
                  sizeof(evac_mlp_policy_t) == offsetof(evac_mlp_policy_t, actor_w1) + kMlpTensors * sizeof(float*) &&
                  offsetof(evac_mlp_policy_t, critic_b3) == offsetof(evac_mlp_policy_t, actor_w1) + (kMlpTensors - 1) * sizeof(float*),
              "the helpers below walk both structs as 13 consecutive pointers, actor_w1 first and critic_b3 last");
inline const float* const* mlp_tensors(const evac_mlp_policy_t& p) { return &p.actor_w1; }
inline float* const* mlp_tensors(const evac_mlp_policy_grads_t& g) { return &g.actor_w1; }
template <class T>
inline bool mlp_all_set(const T& set) {
    for (int i = 0; i < kMlpTensors; ++i)
        if (!mlp_tensors(set)[i]) return false;
    return true;
}

// Their element counts at observation width D (hidden width 64, the only one the kernels take), in the same order.
constexpr int kMlpHidden = 64;
struct MlpSizes {
    int64_t n[kMlpTensors];
};
inline MlpSizes mlp_sizes(int64_t D) {
    const int64_t H = kMlpHidden;
    return {{H * D, H, H * H, H, 2 * H, 2, 2, H * D, H, H * H, H, H, 1}};
}
// A population's strides into `out`: learner s + 1's tensor lies at least one tensor beyond learner s's (a stride of 0 would
// make the learners share it).
inline bool mlp_strides_ok(const evac_mlp_policy_strides_t* st, int32_t obs_dim, int32_t n_learners, int64_t* out) {
    const MlpSizes least = mlp_sizes(obs_dim);
    for (int i = 0; i < kMlpTensors; ++i) {
        out[i] = (&st->actor_w1)[i];
        if (n_learners > 1 && out[i] < least.n[i]) return false;
    }
    return true;
}
// A policy against a handle's observation width, for the entries that run it on a handle's envs (Args: evac::PolicyArgs, which
// starts with the 13 pointers).  Empty and the pointers in `a` (the rest of it zero), or what is refused: the text that follows
// the entry's name in its message.  The entry reports it through its own fail.
template <class Args>
inline std::string mlp_policy_check(const evac_mlp_policy_t& P, int32_t obs_dim, Args& a) {
    if (!mlp_all_set(P)) return ": a tensor pointer of the policy is NULL";
    if (P.hidden != kMlpHidden) return ": hidden must be 64";
    if (P.obs_dim != obs_dim) return ": policy obs_dim " + std::to_string(P.obs_dim) + " != evac_obs_dim " + std::to_string(obs_dim);
    a = Args{P.actor_w1, P.actor_b1, P.actor_w2, P.actor_b2, P.actor_w3, P.actor_b3, P.actor_logstd,
             P.critic_w1, P.critic_b1, P.critic_w2, P.critic_b2, P.critic_w3, P.critic_b3};
    return {};
}

// The instantiation of kernel template K over two or three bools that are known at run time (grav, norm, def of the callers).
#define EVAC_PICK_BOOL2(K, b0, b1) ((b0) ? ((b1) ? K<true, true> : K<true, false>) : ((b1) ? K<false, true> : K<false, false>))
#define EVAC_PICK_BOOL3(K, b0, b1, b2)                                                                                            \
    ((b0) ? ((b1) ? ((b2) ? K<true, true, true> : K<true, true, false>) : ((b2) ? K<true, false, true> : K<true, false, false>)) \
          : ((b1) ? ((b2) ? K<false, true, true> : K<false, true, false>) : ((b2) ? K<false, false, true> : K<false, false, false>)))

// evac_learner_hyper_t [n_learners] (include/evac.h), for every entry that takes one: what the lone entries refuse of the same
// values, for every learner.  (!(x > 0) also refuses a NaN.)
inline bool learner_hypers_ok(const evac_learner_hyper_t* hypers, int32_t n_learners) {
    if (!hypers || n_learners < 1 || n_learners > EVAC_MAX_LEARNERS) return false;
    const auto finite = [](double x) { return x - x == 0.0; };
    for (int s = 0; s < n_learners; ++s) {
        const evac_learner_hyper_t& y = hypers[s];
        if (!finite(y.learning_rate) || !finite(y.gamma) || !finite(y.gae_lambda)) return false;
        if (!(y.max_grad_norm > 0.0f) || !(y.clip_coef >= 0.0f) || !(y.rpo_alpha >= 0.0f)) return false;
        if (y.use_target_kl && y.target_kl != y.target_kl) return false;
    }
    return true;
}

}  // namespace
