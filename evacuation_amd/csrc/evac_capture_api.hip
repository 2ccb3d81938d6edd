// The recording evaluation (include/evac.h: evac_policy_evaluate_capture, evac_policy_evaluate_deepsets_capture,
// evac_policy_evaluate_transformer_capture): policy_evaluate_body (evac_evaluate.h) with the capture policy EvalCapture, for the
// four agent kinds.  A diagnostic face in a unit of its own: the evaluation kernels of evac_api.hip, evac_deepsets_api.hip and
// evac_transformer_api.hip carry none of it.  Only the generic configuration is instantiated (no DEF kernels: the default
// configuration's constants are bit-identical to the handle's own values).  The host side is evac_handle_host.h's: the encoder
// entries are encoder_evaluate<Enc, true>, the linear entry repeats evac_policy_evaluate's checks in their order.
#include <hip/hip_runtime.h>

#include <cstddef>
#include <cstdint>
#include <string>

#define EVAC_TEMPLATE_KERNELS_ONLY      // (evac_device.h: its plain kernels live in evac_api.hip)
#include "evac_deepsets.h"
#include "evac_transformer.h"
#include "evac_deepsets_host.h"
#include "evac_handle_host.h"
#include "evac_host.h"
#include "evac_transformer_env_host.h"

static_assert(sizeof(evac::Params) + sizeof(evac::PolicyArgs) + sizeof(evac::EvalArgs) + sizeof(evac::TransformerArgs) +
                  sizeof(evac::EvalCaptureArgs) <= 4096, "k_evaluate_capture_transformer: arguments beyond the kernel-argument segment");
static_assert(sizeof(evac::PolicyFamily::Smem) + sizeof(evac::PolicySmem<false>) + sizeof(evac::EvalSmem) + sizeof(evac::EvalCaptureSmem) +
                  sizeof(evac::TransformerSmem) <= 160 * 1024, "the capturing kernels' LDS beyond a CU's 160 KiB");
static_assert(sizeof(evac_eval_capture_t) == 24, "evac_eval_capture_t: two counts and two pointers");

namespace evac {

template <bool GRAV, bool NORM>
__global__ __launch_bounds__(PolicyFamily::kBlock, 4) void k_evaluate_capture(Params p, PolicyArgs a, EvalArgs ev, EvalCaptureArgs ca) {
    __shared__ PolicyFamily::Smem sm;
    __shared__ PolicySmem<GRAV> ps;
    __shared__ EvalSmem es;
    __shared__ EvalCaptureSmem cs;
    policy_evaluate_body<true, GRAV, NORM, NoEncoder, false, EvalCapture>(sm, &ps, es, p, a, ev, NoEncoder{}, 0, 0, 0, EvalCapture{cs, ca});
}

__global__ __launch_bounds__(PolicyFamily::kBlock, 4) void k_evaluate_capture_scripted(Params p, EvalArgs ev, EvalCaptureArgs ca) {
    __shared__ PolicyFamily::Smem sm;
    __shared__ EvalSmem es;
    __shared__ EvalCaptureSmem cs;
    policy_evaluate_body<false, false, false, NoEncoder, false, EvalCapture>(sm, (PolicySmem<false>*)nullptr, es, p, PolicyArgs{}, ev,
                                                                             NoEncoder{}, 0, 0, 0, EvalCapture{cs, ca});
}

template <bool NORM>
__global__ __launch_bounds__(PolicyFamily::kBlock, 4) void k_evaluate_capture_deepsets(Params p, PolicyArgs a, EvalArgs ev, DeepSetsArgs da,
                                                                                       EvalCaptureArgs ca) {
    __shared__ PolicyFamily::Smem sm;
    __shared__ PolicySmem<false> ps;
    __shared__ EvalSmem es;
    __shared__ EvalCaptureSmem cs;
    __shared__ DeepSetsSmem ds;
    policy_evaluate_body<true, false, NORM, DeepSetsEncoder, false, EvalCapture>(sm, &ps, es, p, a, ev, DeepSetsEncoder{ds, da}, 0, 0, 0,
                                                                                 EvalCapture{cs, ca});
}

template <bool NORM>
__global__ __launch_bounds__(PolicyFamily::kBlock, 4) void k_evaluate_capture_transformer(Params p, PolicyArgs a, EvalArgs ev,
                                                                                          TransformerArgs ta, EvalCaptureArgs ca) {
    __shared__ PolicyFamily::Smem sm;
    __shared__ PolicySmem<false> ps;
    __shared__ EvalSmem es;
    __shared__ EvalCaptureSmem cs;
    __shared__ TransformerSmem ts;
    policy_evaluate_body<true, false, NORM, TransformerEncoder, false, EvalCapture>(sm, &ps, es, p, a, ev, TransformerEncoder{ts, ta}, 0, 0,
                                                                                    0, EvalCapture{cs, ca});
}

}  // namespace evac

namespace {

// evac_handle_host.h's trait of an encoder, for encoder_evaluate<Enc, true> alone (this unit has no collection entries)
struct DeepSetsCapture : DeepSetsEncoderHost {
    static constexpr const char* kCapture = "evac_policy_evaluate_deepsets_capture";
    static auto capture_kernel(bool norm) { return norm ? evac::k_evaluate_capture_deepsets<true> : evac::k_evaluate_capture_deepsets<false>; }
};
struct TransformerCapture : TransformerEncoderHost {
    static constexpr const char* kCapture = "evac_policy_evaluate_transformer_capture";
    static auto capture_kernel(bool norm) {
        return norm ? evac::k_evaluate_capture_transformer<true> : evac::k_evaluate_capture_transformer<false>;
    }
};

}  // namespace

extern "C" {

// evac_policy_evaluate's checks in its order (evac_api.hip: policy_evaluate without learners), then the capture's.
int evac_policy_evaluate_capture(evac_handle_t h, int32_t agent, const evac_mlp_policy_t* policy, int32_t n_episodes, int32_t max_steps,
                                 int32_t* progress, evac_episode_stats_t* episodes_out, const double* norm_state, float obs_clip,
                                 float epsilon, const evac_eval_capture_t* capture, void* stream) {
    using evac_host::handle_fail;
    const std::string w = "evac_policy_evaluate_capture";
    evac_host::HandleView v;
    if (const int rc = evac_host::handle_begin(h, w.c_str(), &v); rc != EVAC_OK) return rc;
    const bool scripted = agent == EVAC_AGENT_VACUUM_CLEANER;
    if (agent != EVAC_AGENT_POLICY_MEAN && agent != EVAC_AGENT_POLICY_SAMPLE && !scripted)
        return handle_fail(h, EVAC_ERR_INVALID_ARGUMENT, w + ": unknown agent " + std::to_string(agent));
    evac::EvalArgs ev{};
    evac::PolicyArgs a{};
    evac::EvalCaptureArgs ca{};
    std::string why = evaluate_check(agent, n_episodes, max_steps, progress, episodes_out, norm_state, obs_clip, epsilon, ev);
    if (why.empty() && !scripted) why = policy ? mlp_policy_check(*policy, v.p.obs_dim, a) : ": a policy agent needs a policy";
    if (!why.empty()) return handle_fail(h, EVAC_ERR_INVALID_ARGUMENT, w + why);
    if (!(why = one_wave_check(v.p)).empty()) return handle_fail(h, EVAC_ERR_UNSUPPORTED, w + why);
    if (!(why = capture_check(capture, v.p.n_envs, ca)).empty()) return handle_fail(h, EVAC_ERR_INVALID_ARGUMENT, w + why);
    if (const int st = evac_host::handle_settle(h, (hipStream_t)stream); st != EVAC_OK) return st;
    DeviceGuard g(v.device);
    evac_host::handle_turning_points(h, &ev.thr_x, &ev.thr_y);
    const dim3 grid((unsigned)policy_wgs(v.p.n_envs)), block(evac::PolicyFamily::kBlock);
    if (scripted) {
        hipLaunchKernelGGL(evac::k_evaluate_capture_scripted, grid, block, 0, (hipStream_t)stream, v.p, ev, ca);
    } else {
        const auto fn = EVAC_PICK_BOOL2(evac::k_evaluate_capture, v.p.obs_pos == EVAC_POS_GRAV, norm_state != nullptr);
        hipLaunchKernelGGL(fn, grid, block, 0, (hipStream_t)stream, v.p, a, ev, ca);
    }
    return evac_host::handle_check_launch(h, w.c_str());
}

int evac_policy_evaluate_deepsets_capture(evac_handle_t h, int32_t agent, const evac_mlp_policy_t* policy, int32_t n_episodes,
                                          int32_t max_steps, int32_t* progress, evac_episode_stats_t* episodes_out,
                                          const double* norm_state, float obs_clip, float epsilon, const evac_deepsets_t* encoder,
                                          const evac_eval_capture_t* capture, void* stream) {
    return encoder_evaluate<DeepSetsCapture, true>(h, agent, policy, n_episodes, max_steps, progress, episodes_out, norm_state, obs_clip,
                                                   epsilon, encoder, stream, capture);
}

int evac_policy_evaluate_transformer_capture(evac_handle_t h, int32_t agent, const evac_mlp_policy_t* policy, int32_t n_episodes,
                                             int32_t max_steps, int32_t* progress, evac_episode_stats_t* episodes_out,
                                             const double* norm_state, float obs_clip, float epsilon, const evac_transformer_t* encoder,
                                             const evac_eval_capture_t* capture, void* stream) {
    return encoder_evaluate<TransformerCapture, true>(h, agent, policy, n_episodes, max_steps, progress, episodes_out, norm_state,
                                                      obs_clip, epsilon, encoder, stream, capture);
}

}  // extern "C"
