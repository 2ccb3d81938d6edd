// Host side of the deep-sets leader's training entries, the part its translation units share (evac_deepsets_train_api.hip: the
// gradient; evac_deepsets_update_api.hip: the gradient with the optimiser, and the whole update; evac_deepsets_population_api.hip:
// a population's update): the workspace's layout, what the entries check of the encoder, its fields of the kernels' argument
// struct and the encoder's launches in front of and behind the actor-critic's, as the trait SetGrad of
// evac_encoder_train_host.h's templates.
#pragma once

#include "evac_deepsets_train.h"
#include "evac_encoder_train_host.h"

static_assert(evac::kSetTrainHidden == kSetEncoderHidden && evac::kSetTrainMaxElemDim == kSetEncoderMaxElemDim,
              "deepsets_check: the widths the gradient's kernels take, which are the rollout's (evac_deepsets_api.hip asserts its own)");

namespace {

// The deep-sets leader's side of evac_encoder_train_host.h's templates.
struct SetGrad {
    using Encoder = evac_deepsets_t;
    using Grads = evac_deepsets_grads_t;
    using Args = evac::SetArgs;
    using LearnerStrides = evac::SetLearnerStrides;       // (a population's: behind the gate in `tail`)

    // The workspace: evac_rpo_minibatch_grad's own (for a batch of M rows of D floats) | tickets and slots | Y | dY | s | t | the
    // gathered actions, log-probabilities, advantages, returns, values | the index vector | the partials | the dW_r segments;
    // every part on a 256-byte boundary.
    struct Layout {
        int64_t header, Y, dY, sv, tv;
        GatheredLayout cols;
        int64_t parts, rparts, total;
    };
    static Layout layout(int32_t D, int64_t M) {
        Layout L;
        WsCursor c = encoder_ws_cursor(D, M);
        const int64_t f = (int64_t)sizeof(float);
        L.header = c.take(evac::kSetHeaderBytes);
        L.Y = c.take(M * D * f);
        L.dY = c.take(M * D * f);
        L.sv = c.take(M * evac::kSetTrainHidden * f);
        L.tv = c.take(M * evac::kSetTrainHidden * f);
        L.cols = take_gathered(c, M);
        L.parts = c.take((int64_t)evac::set_parts(M) * evac::kSetPart * f);
        const int64_t tiles = (D + evac::kSetRTile - 1) / evac::kSetRTile;
        L.rparts = c.take(tiles * evac::set_segments(M) * evac::kSetRRows * evac::kSetRTile * f);
        L.total = c.o;
        return L;
    }

    // What evac_deepsets_minibatch_grad checks of the encoder behind rpo_prepare's checks, and the encoder's fields of SetArgs.
    static int check(const Encoder& E, const Grads& G, int D, Args& s) {
        if (!G.phi_w1 || !G.phi_b1 || !G.phi_w2 || !G.phi_b2 || !G.rho_w || !G.rho_b) return EVAC_ERR_INVALID_ARGUMENT;
        const int ed = E.set_elem_dim;
        const bool rows_fit = ed > 0 && D % ed == 0 && D / ed >= 3;             // (N + 2 rows, N >= 1)
        if (!deepsets_check(E, D, 0, rows_fit).empty()) return EVAC_ERR_INVALID_ARGUMENT;
        s = Args{};
        s.phi_w1 = E.phi_w1; s.phi_b1 = E.phi_b1; s.phi_w2 = E.phi_w2; s.phi_b2 = E.phi_b2; s.rho_w = E.rho_w; s.rho_b = E.rho_b;
        s.g_phi_w1 = G.phi_w1; s.g_phi_b1 = G.phi_b1; s.g_phi_w2 = G.phi_w2; s.g_phi_b2 = G.phi_b2; s.g_rho_w = G.rho_w; s.g_rho_b = G.rho_b;
        s.D = D; s.ed = ed; s.S = D / ed;
        return EVAC_OK;
    }
    // The encoder's own parts of the workspace and the fields that depend on the minibatch's size.
    static void shape(Args& s, const Layout& L, char* ws, int64_t M) {
        s.dY = (float*)(ws + L.dY); s.sv = (float*)(ws + L.sv); s.tv = (float*)(ws + L.tv);
        s.rparts = (float*)(ws + L.rparts);
        const int p0 = evac::set_parts(M);
        s.chunk = (int)((M + p0 - 1) / p0);
        s.chunk = (s.chunk + evac::kSetTile - 1) / evac::kSetTile * evac::kSetTile;   // whole tiles: every workgroup but the last
        s.P = (int)((M + s.chunk - 1) / s.chunk);                                     // (P <= p0: the workspace's bound)
        s.Sr = evac::set_segments(M);
        s.seglen = (int)((M + s.Sr - 1) / s.Sr);
    }

    // The encoder's launches of one minibatch's gradient, in front of the actor-critic's (the encoder forwards) and behind them
    // (the encoder backwards, its finish): a grid of `y` rows, one per learner; `tail` is what the kernels take behind `s`.
    template <class... Tail>
    static void encode(const Args& s, unsigned y, hipStream_t S, Tail... tail) {
        const int64_t enc_wgs = (s.M + evac::kSetWaves - 1) / evac::kSetWaves;
        hipLaunchKernelGGL(evac::k_set_encode<Tail...>, dim3((unsigned)(enc_wgs > evac::kSetEncodeMaxWgs ? evac::kSetEncodeMaxWgs : enc_wgs), y),
                           dim3(evac::kSetBlock), 0, S, s, tail...);
    }
    template <class... Tail>
    static void backward(const Args& s, unsigned y, hipStream_t S, Tail... tail) {
        hipLaunchKernelGGL(evac::k_set_backward<Tail...>, dim3((unsigned)s.P, y), dim3(evac::kSetBlock), 0, S, s, tail...);
        const int rtiles = (s.D + evac::kSetRTile - 1) / evac::kSetRTile;
        hipLaunchKernelGGL(evac::k_set_finish<Tail...>, dim3((unsigned)(rtiles * s.Sr + 1), y), dim3(evac::kSetBlock), 0, S, s, tail...);
    }
};

}  // namespace
