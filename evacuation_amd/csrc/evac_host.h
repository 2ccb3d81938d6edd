// Host-only helpers shared by the six translation units of libevac: which device a call runs on; the 13 tensors of the
// actor-critic as an array, their sizes, the check of a population's strides, of a policy against a handle and of a set encoder's
// struct; the picker of a kernel template's instantiation over bools; what every entry refuses of evac_learner_hyper_t.
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
// starts with the 13 pointers).  Empty and the pointers in `a` (the rest of it as it was), or what is refused: the text that
// follows the entry's name in its message.  The entry reports it through its own fail.
template <class Args>
inline std::string mlp_policy_check(const evac_mlp_policy_t& P, int32_t obs_dim, Args& a) {
    if (!mlp_all_set(P)) return ": a tensor pointer of the policy is NULL";
    if (P.hidden != kMlpHidden) return ": hidden must be 64";
    if (P.obs_dim != obs_dim) return ": policy obs_dim " + std::to_string(P.obs_dim) + " != evac_obs_dim " + std::to_string(obs_dim);
    a.aw1 = P.actor_w1; a.ab1 = P.actor_b1; a.aw2 = P.actor_w2; a.ab2 = P.actor_b2; a.aw3 = P.actor_w3; a.ab3 = P.actor_b3;
    a.logstd = P.actor_logstd;
    a.cw1 = P.critic_w1; a.cb1 = P.critic_b1; a.cw2 = P.critic_w2; a.cb2 = P.critic_b2; a.cw3 = P.critic_w3; a.cb3 = P.critic_b3;
    return {};
}

// evac_deepsets_t for every entry that takes one: six pointers, the hidden width and the element width the kernels take
// (evac_deepsets.h and evac_deepsets_train.h assert theirs against these), rho_w's alignment.  `rows_fit` is the entry's own
// condition on set_elem_dim x rows = the observation (a handle has its N; the gradient has none); `n_ped` serves the message.
constexpr int kSetEncoderHidden = 24, kSetEncoderMaxElemDim = 6;
inline std::string deepsets_check(const evac_deepsets_t& S, int32_t obs_dim, int32_t n_ped, bool rows_fit) {
    if (!S.phi_w1 || !S.phi_b1 || !S.phi_w2 || !S.phi_b2 || !S.rho_w || !S.rho_b) return ": a tensor pointer of the encoder is NULL";
    if (S.hidden != kSetEncoderHidden) return ": the encoder's hidden must be " + std::to_string(kSetEncoderHidden);
    if (S.set_elem_dim < 1 || S.set_elem_dim > kSetEncoderMaxElemDim || !rows_fit)
        return ": set_elem_dim " + std::to_string(S.set_elem_dim) + " x (" + std::to_string(n_ped) + " + 2) elements is not the observation's " +
               std::to_string(obs_dim) + " floats (a Box observation is needed)";
    if ((uintptr_t)S.rho_w & 15u) return ": rho_w must be 16-byte aligned";
    return {};
}

// A population's strides of the set encoder's six tensors into `out` (evac_deepsets_strides_t, for obs_dim D and element width
// ed): as mlp_strides_ok, and rho_w's rows stay 16-byte aligned in every learner (its stride a multiple of 4 floats).
inline bool deepsets_strides_ok(const evac_deepsets_strides_t* st, int32_t obs_dim, int32_t set_elem_dim, int32_t n_learners, int64_t* out) {
    const int64_t H = kSetEncoderHidden, D = obs_dim;
    const int64_t least[6] = {H * set_elem_dim, H, H * H, H, D * H, D};
    for (int i = 0; i < 6; ++i) {
        out[i] = (&st->phi_w1)[i];
        if (n_learners > 1 && out[i] < least[i]) return false;
    }
    return n_learners <= 1 || out[4] % 4 == 0;
}
static_assert(sizeof(evac_deepsets_strides_t) == 6 * sizeof(int64_t) && offsetof(evac_deepsets_strides_t, rho_b) == 5 * sizeof(int64_t),
              "deepsets_strides_ok walks the struct as 6 consecutive strides, phi_w1 first and rho_b last");

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
