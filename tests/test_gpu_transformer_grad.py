"""GPU tests of the transformer leader's gradient (evac_transformer_minibatch_grad, trainer.transformer_minibatch_grad): all
13 + 16 per block tensors and the 8 statistics against the float64 yardstick of tests/transformer_grad_cases.py, with the method of
tests/test_gpu_deepsets_grad.py -- per tensor err = max|g - g64| / max|g64| (the two key biases, whose exact gradient is zero,
against their weight's largest gradient, a tensor whose float64 gradient vanishes against the case's largest:
transformer_grad_cases.gradient_scales), the bound per case 4 x (torch float32's own largest error on the same case, measured in
the test) + 1e-7, for the tensors and for the statistics.  Then determinism and the written-not-accumulated contract, the
device-drawn perturbation, the sum of squares, the blocks not in use, graph capture, RPOTrainer's wiring and the example.
Everything is compared at the gradient: nothing after an optimiser step.  The table is printed (run with -s) and copied into
DESIGN.md section 4.15."""
import os
import re

import pytest

from tests import encoder_grad_cases as G
from tests import transformer_grad_cases as TC
from tests.encoder_grad_cases import ROOT, ea  # noqa: F401  (the fixture)
from tests.test_gpu_trainer import assert_branch_shares
from tests.trainer_cases import DEV, loss_cfg

pytestmark = pytest.mark.gpu
FACTOR = 4


def kernel_constant(name):
    text = open(os.path.join(ROOT, "evacuation_amd", "csrc", "evac_transformer_train.h")).read()
    return int(re.search(rf"constexpr int {name} = (\d+);", text).group(1))


# the backward kernel's workgroups at their cap: 512 workgroups of 33 samples
CAP_M = kernel_constant("kTfgMaxParts") * (kernel_constant("kTfgSamplesPerWg") + 1)
#        N   ed  M   blocks resid  mode   norm_adv clip_vloss ent   alpha
CASES = [(1, 2, 64, 1, False, "repeat", 0, 1, 0.01, 0.5),           # three tokens
         (1, 6, 1, 1, True, "repeat", 0, 0, 0.0, 0.5),              # M = 1, without norm_adv
         (10, 3, 2, 1, True, "repeat", 1, 1, 0.0, 0.5),             # M = 2, with norm_adv
         (10, 3, 64, 2, False, "strided", 0, 0, 0.01, 0.0),
         (31, 2, 1000, 2, False, "strided", 1, 0, 0.0, 0.0),        # half a wave; M is no multiple of any tile
         (62, 6, 64, 2, False, "repeat", 1, 1, 0.01, 0.0),          # all 64 lanes
         (62, 6, 300, 2, True, "strided", 0, 1, 0.01, 0.0),
         (60, 6, 2048, 2, True, "repeat", 1, 1, 0.01, 0.5),         # the workload's token count; several workgroups
         (10, 3, CAP_M, 2, True, "strided", 1, 0, 0.0, 0.5)]        # the partials at their cap
BIG = CASES[7]


def case_seed(N, ed, M):
    return N + ed + M + 2


def test_the_cases_cover_every_axis():
    assert CAP_M == 16896 and CAP_M > kernel_constant("kTfgMaxParts") * kernel_constant("kTfgSamplesPerWg")
    assert [c[:6] for c in CASES] == [(1, 2, 64, 1, False, "repeat"), (1, 6, 1, 1, True, "repeat"), (10, 3, 2, 1, True, "repeat"),
                                      (10, 3, 64, 2, False, "strided"), (31, 2, 1000, 2, False, "strided"),
                                      (62, 6, 64, 2, False, "repeat"), (62, 6, 300, 2, True, "strided"),
                                      (60, 6, 2048, 2, True, "repeat"), (10, 3, CAP_M, 2, True, "strided")]
    for ed in (2, 3, 6):
        rows = [c for c in CASES if c[1] == ed]
        assert {c[6] for c in rows} == {0, 1} and {c[7] for c in rows} == {0, 1}
        assert {c[8] for c in rows} == {0.0, 0.01} and {c[9] for c in rows} == {0.0, 0.5}
        assert not any(c[4] for c in rows if ed == 2)                 # (two channels with use_resid: under the variance floor)
    assert {(c[6], c[7]) for c in CASES} == {(0, 0), (0, 1), (1, 0), (1, 1)}
    assert {c[3] for c in CASES} == {1, 2} and {c[4] for c in CASES} == {False, True}


ENC = G.Encoder(TC, lambda n: TC.names((n - 13) // 16), lambda got, g64: TC.tensor_errors(got, g64, (len(g64) - 13) // 16),
                "transformer_minibatch_grad", "transformer_kernel_grad", "TransformerActorCritic", "transformer", FACTOR, 20)


@pytest.mark.parametrize("N,ed,M,blocks,resid,mode,norm_adv,clip_vloss,ent,alpha", CASES)
def test_minibatch_grad_against_the_float64_yardstick(ea, N, ed, M, blocks, resid, mode, norm_adv, clip_vloss, ent, alpha):
    cfg = loss_cfg(norm_adv, clip_vloss, ent, alpha)
    net, batch, inds, z, g64, s64, t = TC.build_case(N, ed, M, blocks, resid, mode, cfg, seed=case_seed(N, ed, M))
    assert_branch_shares(t, cfg, M)
    TC.assert_key_biases_are_zero(g64, blocks)
    if mode == "repeat" and M >= 64:
        assert int(inds.unique().numel()) < M                                 # indices do repeat
    g32, s32, _ = TC.minibatch_grad(net, batch, inds, cfg, z)                 # torch, float32, on the GPU
    gk, sk = TC.kernel_grad(net, batch, inds, cfg, z)
    assert len(gk) == 13 + 16 * blocks
    G.check_against_float64(ENC, gk, sk, g32, s32, g64, s64,
                            f"case N={N} ed={ed} M={M} blocks={blocks} resid={int(resid)} {mode} norm_adv={norm_adv} "
                            f"clip_vloss={clip_vloss} ent={ent} alpha={alpha}")


def big_case():
    N, ed, M, blocks, resid, mode, norm_adv, clip_vloss, ent, alpha = BIG
    cfg = loss_cfg(norm_adv, clip_vloss, ent, alpha)
    return (cfg,) + TC.build_case(N, ed, M, blocks, resid, mode, cfg, seed=case_seed(N, ed, M))


def test_deterministic_and_written_not_accumulated(ea):
    G.check_deterministic_and_written_not_accumulated(ENC, *big_case()[:5])


def test_the_encoder_matters(ea):
    cfg, net, batch, inds, z, *_ = big_case()
    gk, sk = TC.kernel_grad(net, batch, inds, cfg, z)
    assert len(gk) == 45
    for i, (name, g) in enumerate(zip(TC.names(2), gk)):
        if i not in TC.key_biases(2):
            assert float(g.abs().max()) > 0, name
    sumsq = float(sum((g.double() ** 2).sum() for g in gk))
    assert abs(float(sk[7]) - sumsq) <= 1e-5 * sumsq, (float(sk[7]), sumsq)


def test_a_block_that_is_not_in_use_is_neither_read_nor_written(ea):
    """With num_blocks = 1 the second block's gradient pointers may be NULL -- trainer.transformer_minibatch_grad leaves them so --
    and the call gives the bits it gives with them set to a buffer, which keeps its contents."""
    import ctypes as C
    import torch
    from evacuation_amd import _lib, trainer
    cfg = loss_cfg(1, 1, 0.0, 0.5)
    net, batch, inds, z, *_ = TC.build_case(10, 3, 2, 1, True, "repeat", cfg, seed=case_seed(10, 3, 2))
    g1, s1 = TC.kernel_grad(net, batch, inds, cfg, z)
    st = trainer._grad_state(net)
    enc, enc_grads = st.binder.transformer(net), trainer.ensure_encoder_grads(net)
    assert enc.num_blocks == 1 and all(getattr(enc_grads.blocks[1], f) is None for f in TC.BLOCK_NAMES)
    assert all(getattr(enc.blocks[1], f) is None for f in TC.BLOCK_NAMES)
    canary = torch.full((16, 128), 3.0, device=DEV)
    set_too = _lib.EvacTransformerGrads()
    set_too.blocks[0] = enc_grads.blocks[0]
    set_too.blocks[1] = _lib.EvacTransformerBlockGrads(*[canary[i].data_ptr() for i in range(16)])
    for p in TC.all_tensors(net):
        p.grad.zero_()
    stats = torch.zeros(8, device=DEV)
    lc = trainer._loss_config(cfg)
    M = int(inds.shape[0])
    rc = _lib.load().evac_transformer_minibatch_grad(
        C.byref(st.binder(net)), C.byref(enc), C.byref(lc), batch["b_obs"].shape[0], *[batch[k].data_ptr() for k in trainer.BATCH_KEYS],
        M, inds.data_ptr(), z.data_ptr(), 0, 0, C.byref(trainer.ensure_grads(net)), C.byref(set_too), stats.data_ptr(),
        st.workspace.data_ptr(), torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    assert rc == 0
    for name, a, p in zip(TC.names(1), g1, TC.all_tensors(net)):
        assert torch.equal(a, p.grad), name
    assert torch.equal(stats, s1) and bool((canary == 3.0).all())


def test_in_place_contract_under_graph_capture(ea):
    cfg = loss_cfg(1, 1, 0.01, 0.5)
    G.check_in_place_contract_under_graph_capture(ENC, cfg, *TC.build_case(10, 3, 64, 2, False, "strided", cfg, seed=21, cache=False)[:4])


def test_trainer_wiring(ea):
    """N = 10, the abs + cat Box observation (D = 36), 8 envs x 16 steps, 2 minibatches x 2 epochs: one update() with
    ``grad_fn = transformer_kernel_grad``, every call recorded, replayed bit for bit and held to float64."""
    import torch
    from evacuation_amd import trainer
    from evacuation_amd.policy import TransformerActorCritic

    def the_device_optimiser_stays_refused(env, net, cfg):
        with pytest.raises(ValueError, match="`embedding`"):
            trainer.RPOTrainer(env, net, cfg, optimizer="device", grad_fn=trainer.transformer_kernel_grad)
    initial, final, calls, cfg = G.check_trainer_wiring(ENC, ea, the_device_optimiser_stays_refused)
    assert len(initial) == 45
    assert sum(not torch.equal(a, b) for a, b in zip(initial, final)) >= 43                           # (all but, at most, the two key biases)
    # what the binder refuses, the entry refuses
    with pytest.raises(ValueError, match="num_heads 2"):
        trainer.transformer_minibatch_grad(TransformerActorCritic(36, 10, num_heads=2).to(DEV), calls[0][1], calls[0][2], cfg)


def test_train_rpo_example_with_the_device_gradient(ea):
    G.check_train_rpo_example_with_the_device_gradient(ENC)
