// Host side and kernels of a SWEEP of a population of deep-sets leaders: a configuration per learner (include/evac.h:
// evac_policy_rollout_sweep_deepsets, evac_deepsets_sweep_workspace_bytes, evac_deepsets_update_sweep).  The unit names its
// kernels and traits; the bodies are shared: collection is evac_handle_host.h's encoder_rollout with the learners' shares and
// their gammas, the sizer and the update are evac_encoder_population_host.h's over SetGrad and SetAdam with the learners'
// values (encoder_update_sweep).  The two kernels are siblings of evac_deepsets_population.h's: the same lines, with the
// learner's gamma / the learner's lr, max_grad_norm and target read at its index.  A unit of its own: the kernel list of
// evac_deepsets_population_api.hip stays what it is.
#include <hip/hip_runtime.h>

#include <cstddef>
#include <cstdint>
#include <string>

#define EVAC_TEMPLATE_KERNELS_ONLY      // (evac_device.h: its plain kernels live in evac_api.hip)
#include "evac_deepsets.h"
#include "evac_deepsets_adam_args.h"
#include "evac_deepsets_train.h"
#include "evac_encoder_sweep.h"
#include "evac_deepsets_adam_host.h"
#include "evac_deepsets_host.h"
#include "evac_encoder_population_host.h"
#include "evac_handle_host.h"
#include "evac_host.h"

namespace evac {

// ---- collection: k_collect_population_deepsets<true, DEF> with the learner's NormalizeReward gamma, as k_collect_sweep
// (evac_policy.h) is k_collect_population's.  Only with the chain does gamma enter collection, hence NORM = true alone.
// TWIN: change one, change the other. ----
template <bool DEF>
__global__ __launch_bounds__(PolicyFamily::kBlock, 4) void k_collect_sweep_deepsets(Params p, int n_steps, PolicyArgs a, NormArgs na,
                                                                                     PopulationArgs q, DeepSetsArgs da, DeepSetsStrides dq,
                                                                                     LearnerGammas lg) {
    __shared__ PolicyFamily::Smem sm;
    __shared__ PolicySmem<false> ps;
    __shared__ DeepSetsSmem ds;
    if constexpr (DEF) p = default_config_constants<false>(p);
    const int s = (int)blockIdx.x / q.wgs;
    const PolicyArgs la = learner_policy(a, q, s);
    da.phi_w1 += s * dq.stride[0]; da.phi_b1 += s * dq.stride[1]; da.phi_w2 += s * dq.stride[2]; da.phi_b2 += s * dq.stride[3];
    da.rho_w += s * dq.stride[4]; da.rho_b += s * dq.stride[5];
    na.gamma = lg.gamma[s];
    // (blockIdx.x x 16 + slot) + shift = s E_l + (blockIdx.x - s wgs) x 16 + slot
    policy_rollout_body<false, true, true, DeepSetsEncoder>(sm, ps, p, n_steps, la, na,
                                                            s * (q.envs_per_learner - q.wgs * PolicyFamily::kEnvsPerBlock),
                                                            (s + 1) * q.envs_per_learner, DeepSetsEncoder{ds, da});
}

// ---- the optimiser step: k_adam_set_population (grid (wg_end[18], S)) whose learner takes lr, max_norm, target_kl and its bit
// of the targets' mask from its entry of the table (evac_encoder_sweep.h).  TWIN of it. ----
__global__ __launch_bounds__(kAdamBlock) void k_adam_set_sweep(SetAdamArgs a, SetAdamStrides q, const LearnerSteps* __restrict__ h) {
    const int64_t s = (int64_t)blockIdx.y;
    const SweepAdamLearner mine = sweep_adam_learner(a, q, h, s);
    if (mine.hdr->stop) return;
    const AdamScalars k = adam_scalars(mine);
    const int b = (int)blockIdx.x;
    int i = 0;
#pragma unroll
    for (int j = 0; j < kSetAdamTensors - 1; ++j) i += b >= a.wg_end[j] ? 1 : 0;
    i = __builtin_amdgcn_readfirstlane(i);      // (0 .. 18 for every workgroup of the grid)
    const int first = i == 0 ? 0 : a.wg_end[i - 1];
    const int o = (b - first) * kAdamBlock + (int)threadIdx.x;
    if (o < a.n[i]) adam_element(mine, k, a.p[i] + s * q.p[i], a.g[i] + s * q.g[i], a.m[i] + s * q.m[i], a.v[i] + s * q.m[i], o);
    adam_close(mine, k);
}

}  // namespace evac

static_assert(sizeof(evac::Params) + 8 + sizeof(evac::PolicyArgs) + sizeof(evac::NormArgs) + sizeof(evac::PopulationArgs) +
                      sizeof(evac::DeepSetsArgs) + sizeof(evac::DeepSetsStrides) + sizeof(evac::LearnerGammas) <= 4096,
              "k_collect_sweep_deepsets: arguments beyond the kernel-argument segment");
static_assert(sizeof(evac::PolicyFamily::Smem) + sizeof(evac::PolicySmem<false>) + sizeof(evac::DeepSetsSmem) <= 160 * 1024,
              "k_collect_sweep_deepsets: LDS beyond a CU's 160 KiB");
static_assert(sizeof(evac::SetAdamArgs) + sizeof(evac::SetAdamStrides) + sizeof(void*) <= 4096,
              "k_adam_set_sweep: arguments beyond the kernel-argument segment");

namespace {

constexpr int kDeepSetsSweepUnit = 0;           // names this unit's k_learner_steps_table

// evac_handle_host.h's trait of an encoder, for the sweep's collection entry
struct DeepSetsSweepEncoder : DeepSetsEncoderHost {
    static constexpr const char* kRollout = "evac_policy_rollout_sweep_deepsets";
};
// ... and its learners: DeepSetsLearnerShares' refusals, then the learners' values; gamma alone is read.  On a raw env (no chain)
// gamma does not enter collection: the population's kernel.
struct DeepSetsSweepLearners : DeepSetsLearnerShares {
    const evac_learner_hyper_t* hypers = nullptr;
    evac::LearnerGammas lg{};

    std::string check(const evac::Params& p, const evac_mlp_policy_t& policy, const evac_deepsets_t& encoder) {
        std::string why = DeepSetsLearnerShares::check(p, policy, encoder);
        if (!why.empty()) return why;
        if (!learner_hypers_ok(hypers, n_learners)) return ": hypers is NULL or a learner's values are refused (see evac_learner_hyper_t)";
        for (int s = 0; s < n_learners; ++s) lg.gamma[s] = (float)hypers[s].gamma;
        return why;
    }
    void launch(const evac_host::HandleView& v, int n_steps, const evac::PolicyArgs& a, const evac::NormArgs& na,
                const evac::DeepSetsArgs& ea, hipStream_t S) const {
        const dim3 grid((unsigned)(n_learners * q.wgs)), block(evac::PolicyFamily::kBlock);
        if (na.state) {
            const auto fn = v.default_cfg ? evac::k_collect_sweep_deepsets<true> : evac::k_collect_sweep_deepsets<false>;
            hipLaunchKernelGGL(fn, grid, block, 0, S, v.p, n_steps, a, na, q, ea, dq, lg);
        } else {
            evac::deepsets_population_launch_collect(v, n_steps, a, na, n_learners, q, ea, dq, S);
        }
    }
};

}  // namespace

extern "C" {

int evac_policy_rollout_sweep_deepsets(evac_handle_t h, int32_t n_learners, const evac_mlp_policy_t* policy,
                                       const evac_mlp_policy_strides_t* strides, const evac_deepsets_t* encoder,
                                       const evac_deepsets_strides_t* enc_strides, int32_t n_steps, float* next_obs, float* next_done,
                                       float* obs_out, float* actions_out, float* logprob_out, float* value_out, float* reward_out,
                                       float* done_out, float* next_value_out, evac_episode_stats_t* final_stats, double* norm_state,
                                       float gamma, float obs_clip, float reward_clip, float epsilon, const evac_learner_hyper_t* hypers,
                                       void* stream) {
    DeepSetsSweepLearners learners{{n_learners, strides, enc_strides}};
    learners.hypers = hypers;
    return encoder_rollout<DeepSetsSweepEncoder>(h, n_steps, policy,
                                                 collect_outputs(next_obs, next_done, obs_out, actions_out, logprob_out, value_out,
                                                                 reward_out, done_out, next_value_out, final_stats),
                                                 evac::NormArgs{norm_state, gamma, obs_clip, reward_clip, epsilon}, encoder, stream, learners);
}

int64_t evac_deepsets_sweep_workspace_bytes(int32_t obs_dim, int64_t n_minibatch, int32_t n_learners) {
    return encoder_sweep_workspace_bytes<SetGrad>(obs_dim, n_minibatch, n_learners);
}

int evac_deepsets_update_sweep(int32_t n_learners, const evac_mlp_policy_t* policy, const evac_deepsets_t* encoder,
                               const evac_mlp_policy_grads_t* params, const evac_deepsets_grads_t* enc_params,
                               const evac_mlp_policy_grads_t* grads, const evac_deepsets_grads_t* enc_grads,
                               const evac_mlp_policy_strides_t* param_strides, const evac_deepsets_strides_t* enc_param_strides,
                               const evac_mlp_policy_strides_t* grad_strides, const evac_deepsets_strides_t* enc_grad_strides,
                               const evac_mlp_policy_strides_t* moment_strides, const evac_deepsets_strides_t* enc_moment_strides,
                               int64_t header_stride_bytes, const evac_rpo_loss_config_t* loss_cfg, const evac_adam_config_t* adam_cfg,
                               const evac_deepsets_adam_state_t* state, int64_t batch_size, const float* b_obs, const float* b_actions,
                               const float* b_logprobs, const float* b_advantages, const float* b_returns, const float* b_values,
                               int64_t learner_batch_size, int64_t n_minibatch, int32_t n_epochs, const int64_t* perms,
                               const float* rpo_noise, const uint64_t* seeds, const uint64_t* first_draw_counters,
                               const evac_learner_hyper_t* hypers, float* stats_out, void* workspace, void* stream) {
    return encoder_update_sweep<SetGrad, SetAdam, kDeepSetsSweepUnit>(
        evac::k_adam_set_sweep, n_learners, policy, encoder, params, enc_params, grads, enc_grads, param_strides, enc_param_strides,
        grad_strides, enc_grad_strides, moment_strides, enc_moment_strides, header_stride_bytes, loss_cfg, adam_cfg, state, batch_size,
        b_obs, b_actions, b_logprobs, b_advantages, b_returns, b_values, learner_batch_size, n_minibatch, n_epochs, perms, rpo_noise,
        seeds, first_draw_counters, hypers, stats_out, workspace, stream);
}

}  // extern "C"
