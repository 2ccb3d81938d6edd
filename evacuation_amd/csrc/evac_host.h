// Host-only helpers shared by the translation units of libevac (evac_api.hip: the env; evac_train_api.hip: the trainer's
// update): which device a call runs on, and the 13 tensors of the actor-critic as an array.
#pragma once

#include <hip/hip_runtime.h>
#include <stddef.h>

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
