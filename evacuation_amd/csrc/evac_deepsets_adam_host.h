// Host side of the deep-sets leader's optimiser step, the part its two translation units share (evac_deepsets_update_api.hip:
// one learner; evac_deepsets_population_api.hip: a population): the trait SetAdam of evac_encoder_train_host.h's and
// evac_encoder_population_host.h's templates -- the encoder's six tensors behind the actor-critic's 13, what is refused of their
// sizes and of a population's strides, and the launch.  The kernels stay in the units (k_adam_set, k_adam_set_population): both
// take evac::SetAdamArgs.
#pragma once

#include "evac_deepsets_adam_args.h"
#include "evac_deepsets_train_host.h"

static_assert(sizeof(evac_deepsets_grads_t) == 6 * sizeof(float*) && offsetof(evac_deepsets_grads_t, rho_b) == 5 * sizeof(float*),
              "SetAdam::tensor walks the struct as 6 consecutive pointers, phi_w1 first and rho_b last");
static_assert(offsetof(evac_deepsets_adam_state_t, exp_avg) == offsetof(evac_adam_state_t, exp_avg) &&
                  offsetof(evac_deepsets_adam_state_t, exp_avg_sq) == offsetof(evac_adam_state_t, exp_avg_sq),
              "the state of the 13 tensors is evac_adam_state_t's");

namespace {

// The deep-sets leader's side of the optimiser's templates.
struct SetAdam {
    using State = evac_deepsets_adam_state_t;
    using Grads = evac_deepsets_grads_t;
    using Args = evac::SetAdamArgs;
    using Strides = evac::SetAdamStrides;
    using EncoderStrides = evac_deepsets_strides_t;
    struct Dims {
        int32_t ed;
    };
    static Dims dims(const evac_deepsets_t& E) { return {E.set_elem_dim}; }

    static int check(int32_t D, const Dims& d) {
        if (d.ed < 1 || d.ed > evac::kSetTrainMaxElemDim || D % d.ed != 0 || D / d.ed < 3) return EVAC_ERR_INVALID_ARGUMENT;
        return EVAC_OK;
    }
    static Args fresh(const Dims&) { return Args{}; }
    static int count(const Dims&) { return 6; }
    static float* tensor(const Grads& g, int i) { return (&g.phi_w1)[i]; }
    // evac_deepsets_t: phi_w1 [24][ed], phi_b1 [24], phi_w2 [24][24], phi_b2 [24], rho_w [D][24], rho_b [D]
    static int size(int i, int32_t D, const Dims& d) {
        const int H = evac::kSetTrainHidden;
        const int n[6] = {H * d.ed, H, H * H, H, D * H, D};
        return n[i];
    }
    // One launch of the optimiser's kernel over `learners` learners: `kernel` is k_adam_set (rest: nothing) or
    // k_adam_set_population (rest: its SetAdamStrides); the grid is every tensor's workgroups, times the learners.
    template <class Kernel, class... Rest>
    static void launch(Kernel kernel, const Args& q, unsigned learners, hipStream_t S, const Rest&... rest) {
        hipLaunchKernelGGL(kernel, dim3((unsigned)q.wg_end[evac::kSetAdamTensors - 1], learners), dim3(evac::kAdamBlock), 0, S, q, rest...);
    }

    // A population's strides of the encoder's tensors -- parameters, gradients, moments -- held against the tensors
    // (deepsets_strides_ok) and copied to where the gradient's kernels (`sq`) and the optimiser's (`aq`, behind the 13) read them.
    static bool strides(const evac_deepsets_t& E, int32_t D, int32_t n_learners, const EncoderStrides* p, const EncoderStrides* g,
                        const EncoderStrides* m, evac::SetLearnerStrides& sq, Strides& aq) {
        const int ed = E.set_elem_dim;
        if (!deepsets_strides_ok(p, D, ed, n_learners, sq.p) || !deepsets_strides_ok(g, D, ed, n_learners, sq.g) ||
            !deepsets_strides_ok(m, D, ed, n_learners, aq.m + evac::kAdamTensors))
            return false;
        for (int i = 0; i < 6; ++i) {
            aq.p[evac::kAdamTensors + i] = sq.p[i]; aq.g[evac::kAdamTensors + i] = sq.g[i];
        }
        return true;
    }
};

// evac_deepsets_adam_step's checks and set-up with the encoder's size as the entry takes it.
inline int set_adam_prepare(const evac_mlp_policy_grads_t* params, const evac_deepsets_grads_t* enc_params,
                            const evac_mlp_policy_grads_t* grads, const evac_deepsets_grads_t* enc_grads,
                            const evac_deepsets_adam_state_t* state, const evac_adam_config_t* cfg, int32_t obs_dim, int32_t set_elem_dim,
                            evac::AdamArgs& o, evac::SetAdamArgs& q) {
    return encoder_adam_prepare<SetAdam>(params, enc_params, grads, enc_grads, state, cfg, obs_dim, SetAdam::Dims{set_elem_dim}, o, q);
}

}  // namespace
