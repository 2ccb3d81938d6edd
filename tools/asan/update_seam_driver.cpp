// A stand-alone program for tools/asan_update_seam.sh: the host code that the deep-sets and the transformer leader's optimiser,
// update and population entries share (evac_encoder_train_host.h, evac_encoder_population_host.h, the population preamble of
// evac_handle_host.h), driven with no device through the two population sizers and through every folded entry's refusal paths.
// Every refusal precedes the first HIP call, so the made-up pointers below are never followed; the paths chosen run the shared
// bodies to their LAST check (a NULL second moment), so that the traits' walks over the C structs -- tensors, sizes, strides --
// all run under the sanitizers.  Prints "update seam driver: ok" and returns 0, or names what came back wrong.
#include <cstdint>
#include <cstdio>
#include <initializer_list>

#include "evac.h"

namespace {

int failures = 0;
void expect(int64_t got, int64_t want, const char* what) {
    if (got == want) return;
    std::printf("FAILED: %s: got %lld, expected %lld\n", what, (long long)got, (long long)want);
    ++failures;
}

float* const F = (float*)0x1000;                 // 16-byte aligned, never followed
const int BAD = EVAC_ERR_INVALID_ARGUMENT, UNSUP = EVAC_ERR_UNSUPPORTED;
int64_t round256(int64_t n) { return (n + 255) / 256 * 256; }

template <class T>
void set_all(T& t, float* p) {                   // a struct of nothing but float pointers
    float** f = (float**)&t;
    for (size_t i = 0; i < sizeof(T) / sizeof(float*); ++i) f[i] = p;
}
evac_mlp_policy_t policy_of(int D) { return {D, 64, F, F, F, F, F, F, F, F, F, F, F, F, F}; }
evac_mlp_policy_strides_t mlp_strides(int64_t D) { return {64 * D, 64, 64 * 64, 64, 128, 2, 2, 64 * D, 64, 64 * 64, 64, 64, 1}; }

// What the two encoders' cases share: a call of every folded entry whose arguments are all acceptable, to be spoiled one at a time.
struct Common {
    int S = 2, D = 36, M = 4, B_l = 8, epochs = 2;
    int64_t batch;                               // the common batch: the learners' B_l rows each
    evac_mlp_policy_t pol;
    evac_mlp_policy_grads_t params, grads;
    evac_mlp_policy_strides_t strides[3];
    int64_t header_stride = 64;
    evac_rpo_loss_config_t cfg{0.2f, 0.0f, 0.5f, 0.5f, 1, 1};
    evac_adam_config_t adam{3e-4, 0.9, 0.999, 1e-5, 0.5};
    void* workspace = F;
    uint64_t u64[64] = {};
    // which struct arguments go in as NULL
    bool no_pol = false, no_enc = false, no_params = false, no_enc_params = false, no_grads = false, no_enc_grads = false,
         no_cfg = false, no_adam = false, no_state = false, no_strides[3] = {}, no_enc_strides[3] = {};

    explicit Common(int S_, int D_) : S(S_), D(D_), batch((int64_t)S_ * 8), pol(policy_of(D_)) {
        set_all(params, F);
        set_all(grads, F);
        for (auto& s : strides) s = mlp_strides(D_);
    }
};

struct SetCase : Common {
    evac_deepsets_t enc;
    evac_deepsets_grads_t enc_params, enc_grads;
    evac_deepsets_strides_t enc_strides[3];
    evac_deepsets_adam_state_t state;

    explicit SetCase(int S_ = 2, int D_ = 36, int ed = 3) : Common(S_, D_), enc{ed, 24, F, F, F, F, F, F} {
        set_all(enc_params, F);
        set_all(enc_grads, F);
        for (auto& s : enc_strides) s = {24 * ed, 24, 24 * 24, 24, (int64_t)D_ * 24, D_};
        state.header = F;
        set_all(state.exp_avg, F); set_all(state.exp_avg_sq, F); set_all(state.enc_exp_avg, F); set_all(state.enc_exp_avg_sq, F);
    }
    float*& last_moment() { return state.enc_exp_avg_sq.rho_b; }
    int64_t& a_stride(int which) { return enc_strides[which].phi_w2; }
    int update_population() const {
        return evac_deepsets_update_population(
            S, no_pol ? nullptr : &pol, no_enc ? nullptr : &enc, no_params ? nullptr : &params, no_enc_params ? nullptr : &enc_params,
            no_grads ? nullptr : &grads, no_enc_grads ? nullptr : &enc_grads, no_strides[0] ? nullptr : &strides[0],
            no_enc_strides[0] ? nullptr : &enc_strides[0], no_strides[1] ? nullptr : &strides[1],
            no_enc_strides[1] ? nullptr : &enc_strides[1], no_strides[2] ? nullptr : &strides[2],
            no_enc_strides[2] ? nullptr : &enc_strides[2], header_stride, no_cfg ? nullptr : &cfg, no_adam ? nullptr : &adam,
            no_state ? nullptr : &state, batch, F, F, F, F, F, F, B_l, M, epochs, (const int64_t*)F, nullptr, u64, u64, 1, 0.01, F,
            workspace, nullptr);
    }
    int update() const {
        return evac_deepsets_update(no_pol ? nullptr : &pol, no_enc ? nullptr : &enc, no_params ? nullptr : &params,
                                    no_enc_params ? nullptr : &enc_params, no_grads ? nullptr : &grads, no_enc_grads ? nullptr : &enc_grads,
                                    no_cfg ? nullptr : &cfg, no_adam ? nullptr : &adam, no_state ? nullptr : &state, B_l, F, F, F, F, F, F, M,
                                    epochs, (const int64_t*)F, nullptr, 1, 0, 1, 0.01, F, workspace, nullptr);
    }
    int minibatch_step() const {
        return evac_deepsets_minibatch_step(no_pol ? nullptr : &pol, no_enc ? nullptr : &enc, no_cfg ? nullptr : &cfg, B_l, F, F, F, F, F, F, M,
                                            (const int64_t*)F, nullptr, 1, 0, no_grads ? nullptr : &grads,
                                            no_enc_grads ? nullptr : &enc_grads, F, workspace, nullptr, no_params ? nullptr : &params,
                                            no_enc_params ? nullptr : &enc_params, no_state ? nullptr : &state, no_adam ? nullptr : &adam);
    }
    int adam_step(const float* sumsq) const {
        return evac_deepsets_adam_step(no_params ? nullptr : &params, no_enc_params ? nullptr : &enc_params, no_grads ? nullptr : &grads,
                                       no_enc_grads ? nullptr : &enc_grads, no_state ? nullptr : &state, no_adam ? nullptr : &adam, D,
                                       enc.set_elem_dim, sumsq, nullptr);
    }
};

struct TfCase : Common {
    evac_transformer_t enc;
    evac_transformer_grads_t enc_params{}, enc_grads{};
    evac_transformer_strides_t enc_strides[3] = {};
    evac_transformer_adam_state_t state{};

    explicit TfCase(int S_ = 2, int D_ = 36, int dm = 3, int blocks = 2) : Common(S_, D_), enc{dm, blocks, 3, 96, 0, 1e-5f, {}} {
        const int64_t d = dm;
        state.header = F;
        set_all(state.exp_avg, F); set_all(state.exp_avg_sq, F);
        for (int b = 0; b < blocks && b < 2; ++b) {                  // (the blocks beyond: NULL pointers and zero strides everywhere)
            set_all(enc.blocks[b], F);
            set_all(enc_params.blocks[b], F); set_all(enc_grads.blocks[b], F);
            set_all(state.enc_exp_avg.blocks[b], F); set_all(state.enc_exp_avg_sq.blocks[b], F);
            for (auto& s : enc_strides)
                s.blocks[b] = {3 * d * d, 3 * d, 3 * d * d, 3 * d, 3 * d * d, 3 * d, 3 * d * d, d, 96 * d, 96, 96 * d, d, d, d, d, d};
        }
    }
    float*& last_moment() { return state.enc_exp_avg_sq.blocks[enc.num_blocks - 1].norm2_b; }
    int64_t& a_stride(int which) { return enc_strides[which].blocks[enc.num_blocks - 1].ff1_w; }
    int update_population() const {
        return evac_transformer_update_population(
            S, no_pol ? nullptr : &pol, no_enc ? nullptr : &enc, no_params ? nullptr : &params, no_enc_params ? nullptr : &enc_params,
            no_grads ? nullptr : &grads, no_enc_grads ? nullptr : &enc_grads, no_strides[0] ? nullptr : &strides[0],
            no_enc_strides[0] ? nullptr : &enc_strides[0], no_strides[1] ? nullptr : &strides[1],
            no_enc_strides[1] ? nullptr : &enc_strides[1], no_strides[2] ? nullptr : &strides[2],
            no_enc_strides[2] ? nullptr : &enc_strides[2], header_stride, no_cfg ? nullptr : &cfg, no_adam ? nullptr : &adam,
            no_state ? nullptr : &state, batch, F, F, F, F, F, F, B_l, M, epochs, (const int64_t*)F, nullptr, u64, u64, 1, 0.01, F,
            workspace, nullptr);
    }
    int update() const {
        return evac_transformer_update(no_pol ? nullptr : &pol, no_enc ? nullptr : &enc, no_params ? nullptr : &params,
                                       no_enc_params ? nullptr : &enc_params, no_grads ? nullptr : &grads,
                                       no_enc_grads ? nullptr : &enc_grads, no_cfg ? nullptr : &cfg, no_adam ? nullptr : &adam,
                                       no_state ? nullptr : &state, B_l, F, F, F, F, F, F, M, epochs, (const int64_t*)F, nullptr, 1, 0, 1, 0.01,
                                       F, workspace, nullptr);
    }
    int minibatch_step() const {
        return evac_transformer_minibatch_step(no_pol ? nullptr : &pol, no_enc ? nullptr : &enc, no_cfg ? nullptr : &cfg, B_l, F, F, F, F, F, F,
                                               M, (const int64_t*)F, nullptr, 1, 0, no_grads ? nullptr : &grads,
                                               no_enc_grads ? nullptr : &enc_grads, F, workspace, nullptr, no_params ? nullptr : &params,
                                               no_enc_params ? nullptr : &enc_params, no_state ? nullptr : &state, no_adam ? nullptr : &adam);
    }
    int adam_step(const float* sumsq) const {
        return evac_transformer_adam_step(no_params ? nullptr : &params, no_enc_params ? nullptr : &enc_params, no_grads ? nullptr : &grads,
                                          no_enc_grads ? nullptr : &enc_grads, no_state ? nullptr : &state, no_adam ? nullptr : &adam, D,
                                          enc.elem_dim, enc.num_blocks, sumsq, nullptr);
    }
};

// The refusals the two encoders share, in the shared bodies' order; `Case` is SetCase or TfCase.
template <class Case>
void shared_refusals(const char* who) {
    std::printf("%s\n", who);
    // -- the whole walk, up to the last check of each entry: the optimiser's NULL second moment of the last tensor
    for (int S : {1, 2, 64}) {
        Case c(S);
        c.last_moment() = nullptr;
        expect(c.update_population(), BAD, "update_population: up to the NULL last moment");
    }
    {
        Case c;
        c.last_moment() = nullptr;
        expect(c.update(), BAD, "update: up to the NULL last moment");
        expect(c.minibatch_step(), BAD, "minibatch_step: up to the NULL last moment");
        expect(c.adam_step(F), BAD, "adam_step: up to the NULL last moment");
    }
    expect(Case().adam_step(nullptr), BAD, "adam_step: every tensor accepted, NULL grad_sumsq");
    // -- the population's own, in their order
    for (int S : {0, 65}) expect(Case(S).update_population(), BAD, "update_population: n_learners 0 / 65");
    {
        Case c;
        c.no_state = true;
        expect(c.update_population(), BAD, "update_population: NULL state, in front of population_prepare");
        expect(c.update(), BAD, "update: NULL state");
        expect(c.minibatch_step(), BAD, "minibatch_step: NULL state");
        expect(c.adam_step(F), BAD, "adam_step: NULL state");
    }
    for (int which = 0; which < 3; ++which) {
        for (int S : {1, 2}) {
            Case c(S);
            c.no_enc_strides[which] = true;
            expect(c.update_population(), BAD, "update_population: a NULL encoder strides struct, at S = 1 too");
        }
        Case c;
        c.no_strides[which] = true;
        expect(c.update_population(), BAD, "update_population: a NULL policy strides struct");
        Case e;
        e.a_stride(which) -= 1;
        expect(e.update_population(), BAD, "update_population: an encoder stride below its tensor");
    }
    {
        Case c;
        c.header_stride = 68;
        expect(c.update_population(), BAD, "update_population: header stride 68");
        Case e;
        e.epochs = 0;
        expect(e.update_population(), BAD, "update_population: n_epochs 0");
        expect(e.update(), BAD, "update: n_epochs 0");
    }
    for (int k = 0; k < 7; ++k) {
        Case c;
        (k == 0 ? c.no_pol : k == 1 ? c.no_enc : k == 2 ? c.no_params : k == 3 ? c.no_enc_params : k == 4 ? c.no_grads : k == 5 ? c.no_enc_grads : c.no_adam) = true;
        expect(c.update_population(), BAD, "update_population: a NULL struct");
        expect(c.update(), BAD, "update: a NULL struct");
        expect(c.minibatch_step(), BAD, "minibatch_step: a NULL struct");
        if (k >= 2) expect(c.adam_step(F), BAD, "adam_step: a NULL struct");
    }
}

void sizers() {
    std::printf("sizers\n");
    const int shapes[][2] = {{9, 8}, {36, 70}, {72, 3}, {372, 192}, {384, 1024}};
    for (const auto& dm : shapes) {
        const int D = dm[0];
        const int64_t M = dm[1];
        for (int S : {1, 2, 3, 8, 64}) {
            const int64_t rows = S * M;
            const int64_t common = round256(rows * D * 4) + round256(rows * 2 * 4) + 4 * round256(rows * 4) + round256(rows * 8);
            expect(evac_transformer_population_workspace_bytes(D, M, S), S * round256(evac_transformer_workspace_bytes(D, M)) + common,
                   "transformer sizer: S slices and the common batch");
            if (D % 3 == 0)
                expect(evac_deepsets_population_workspace_bytes(D, M, S), S * round256(evac_deepsets_workspace_bytes(D, M)) + common,
                       "deep-sets sizer: S slices and the common batch");
        }
    }
    const int bad[][3] = {{0, 64, 2}, {397, 64, 2}, {6, 0, 2}, {6, -1, 2}, {36, 64, 0}, {36, 64, -1}, {36, 64, 65}};
    for (const auto& b : bad) {
        expect(evac_transformer_population_workspace_bytes(b[0], b[1], b[2]), BAD, "transformer sizer: refused");
        expect(evac_deepsets_population_workspace_bytes(b[0], b[1], b[2]), BAD, "deep-sets sizer: refused");
    }
}

// Each encoder's own: its size refusals with their codes, and the order of the gradient's checks before the population's.
void own_refusals() {
    std::printf("the encoders' own\n");
    expect(SetCase(2, 42, 7).update_population(), BAD, "deep-sets: set_elem_dim 7");
    expect(SetCase(2, 36, 5).update_population(), BAD, "deep-sets: D no multiple of set_elem_dim");
    expect(SetCase(2, 42, 7).adam_step(F), BAD, "deep-sets adam_step: set_elem_dim 7");
    {
        SetCase c;
        c.enc_strides[2].rho_w += 2;
        expect(c.update_population(), BAD, "deep-sets: rho_w's moment stride no multiple of 4 floats");
    }
    expect(TfCase(2, 3 * 65, 3).update_population(), UNSUP, "transformer: 65 tokens");
    expect(TfCase(2, 3 * 65, 3).adam_step(F), UNSUP, "transformer adam_step: 65 tokens");
    expect(TfCase(2, 42, 7).adam_step(F), BAD, "transformer adam_step: elem_dim 7");
    {
        TfCase c;
        c.enc.num_blocks = 3;
        expect(c.update_population(), UNSUP, "transformer: num_blocks 3");
        expect(c.update(), UNSUP, "transformer update: num_blocks 3");
        expect(evac_transformer_adam_step(&c.params, &c.enc_params, &c.grads, &c.enc_grads, &c.state, &c.adam, 36, 3, 3, F, nullptr), UNSUP,
               "transformer adam_step: num_blocks 3 before elem_dim and the pointers");
        expect(evac_transformer_adam_step(&c.params, &c.enc_params, &c.grads, &c.enc_grads, &c.state, &c.adam, 36, 7, 0, F, nullptr), UNSUP,
               "transformer adam_step: num_blocks 0 before elem_dim 7");
    }
    {
        TfCase c;
        c.enc.num_heads = 4;
        c.no_state = true;
        expect(c.update_population(), UNSUP, "transformer: num_heads 4 and a NULL state: the encoder first");
        TfCase e(0, 3 * 65, 3);
        e.batch = 16;                            // (the common batch itself is acceptable)
        e.a_stride(0) = 0;
        expect(e.update_population(), UNSUP, "transformer: 65 tokens, no learners, a zero stride: the encoder first");
    }
    {
        TfCase c(2, 36, 3, 1);                   // one block: blocks[1] NULL everywhere, its strides below every tensor
        for (auto& s : c.enc_strides) s.blocks[1].wq = -5;
        c.last_moment() = nullptr;
        expect(c.update_population(), BAD, "transformer: one block, blocks[1] never looked at, up to the NULL last moment");
        expect(c.adam_step(nullptr), BAD, "transformer adam_step: one block accepted, NULL grad_sumsq");
    }
}

// The population's collection and evaluation entries: without a handle they are refused before anything else.
void handle_entries() {
    std::printf("collection and evaluation\n");
    SetCase s;
    TfCase t;
    evac_episode_stats_t* const stats = (evac_episode_stats_t*)F;
    for (int null = 0; null < 3; ++null) {
        const evac_mlp_policy_strides_t* st = null == 1 ? nullptr : &s.strides[0];
        const evac_deepsets_strides_t* se = null == 2 ? nullptr : &s.enc_strides[0];
        const evac_transformer_strides_t* te = null == 2 ? nullptr : &t.enc_strides[0];
        expect(evac_policy_rollout_population_deepsets(nullptr, 2, &s.pol, st, &s.enc, se, 4, F, F, F, F, F, F, F, F, F, stats, nullptr, 0.99f,
                                                       10.0f, 10.0f, 1e-8f, nullptr),
               BAD, "deep-sets collection: no handle");
        expect(evac_policy_rollout_population_transformer(nullptr, 2, &t.pol, st, &t.enc, te, 4, F, F, F, F, F, F, F, F, F, stats, nullptr,
                                                          0.99f, 10.0f, 10.0f, 1e-8f, nullptr),
               BAD, "transformer collection: no handle");
        expect(evac_policy_evaluate_population_deepsets(nullptr, 2, &s.pol, st, &s.enc, se, EVAC_AGENT_POLICY_MEAN, 0, 4, 100, (int32_t*)F, stats,
                                                        nullptr, 10.0f, 1e-8f, nullptr),
               BAD, "deep-sets evaluation: no handle");
        expect(evac_policy_evaluate_population_transformer(nullptr, 2, &t.pol, st, &t.enc, te, EVAC_AGENT_POLICY_MEAN, 0, 4, 100, (int32_t*)F,
                                                           stats, nullptr, 10.0f, 1e-8f, nullptr),
               BAD, "transformer evaluation: no handle");
    }
}

}  // namespace

int main() {
    sizers();
    shared_refusals<SetCase>("deep-sets");
    shared_refusals<TfCase>("transformer");
    own_refusals();
    handle_entries();
    if (failures) return std::printf("update seam driver: %d FAILED\n", failures), 1;
    std::printf("update seam driver: ok\n");
    return 0;
}
