// Host side of the deep-sets leader, the part the units that run it on a handle's envs share (evac_deepsets_api.hip: collection
// and evaluation; evac_capture_api.hip: the recording evaluation): the set encoder against the handle, as evac_handle_host.h's
// trait of an encoder asks for it.  A unit derives its trait from this and adds its entries' names and kernels.
#pragma once

#include <cstdint>
#include <string>

#include "evac_deepsets.h"
#include "evac_handle_host.h"
#include "evac_host.h"

static_assert(evac::kSetHidden == kSetEncoderHidden && evac::kSetMaxElemDim == kSetEncoderMaxElemDim,
              "deepsets_check: the widths the deep-sets kernels take");

namespace evac {
// k_collect_population_deepsets on `stream` (evac_deepsets_population_api.hip; the sweep's unit launches it on a raw env, where no
// gamma enters collection): a plain host function, so that the kernel is instantiated in one translation unit alone
void deepsets_population_launch_collect(const evac_host::HandleView& v, int n_steps, const PolicyArgs& a, const NormArgs& na,
                                        int n_learners, const PopulationArgs& q, const DeepSetsArgs& ea, const DeepSetsStrides& dq,
                                        hipStream_t stream);
}  // namespace evac

namespace {

// `check` comes after the policy's thirteen tensors; every refusal of a set encoder is EVAC_ERR_INVALID_ARGUMENT.
struct DeepSetsEncoderHost {
    using Struct = evac_deepsets_t;
    using Args = evac::DeepSetsArgs;
    static int check(const evac::Params& p, const evac_deepsets_t& S, evac::DeepSetsArgs& da, std::string& why) {
        // (the gravity observation's 6 floats are no whole number of rows for any N >= 5, and no set for the others)
        const bool rows_fit = p.obs_pos != EVAC_POS_GRAV && (int64_t)S.set_elem_dim * (p.n_ped + 2) == (int64_t)p.obs_dim;
        da = evac::DeepSetsArgs{S.phi_w1, S.phi_b1, S.phi_w2, S.phi_b2, S.rho_w, S.rho_b, (int)S.set_elem_dim};
        why = deepsets_check(S, p.obs_dim, p.n_ped, rows_fit);
        return why.empty() ? EVAC_OK : EVAC_ERR_INVALID_ARGUMENT;
    }
};

// The learners of a population of such networks, for evac_handle_host.h's Learners of encoder_rollout / encoder_evaluate
// (evac_deepsets_population_api.hip, evac_deepsets_population_evaluate_api.hip): their shares of the handle's envs and the strides
// of their 19 tensors, refused behind the networks.  A unit derives its Learners from this and adds its launch.
struct DeepSetsLearnerShares {
    static constexpr bool kOn = true;
    int32_t n_learners;
    const evac_mlp_policy_strides_t* strides;
    const evac_deepsets_strides_t* enc_strides;
    evac::PopulationArgs q{};
    evac::DeepSetsStrides dq{};

    std::string check(const evac::Params& p, const evac_mlp_policy_t& policy, const evac_deepsets_t& encoder) {
        std::string why = learner_shares(p.n_envs, n_learners, strides, policy.obs_dim, q);
        if (why.empty() && !deepsets_strides_ok(enc_strides, p.obs_dim, encoder.set_elem_dim, n_learners, dq.stride))
            why = ": an encoder stride is smaller than its tensor, or rho_w's is no multiple of 4 floats";
        return why;
    }
};

}  // namespace
