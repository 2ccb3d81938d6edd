"""GPU tests of the deep-sets leader's gradient (evac_deepsets_minibatch_grad, trainer.deepsets_minibatch_grad): all 19 tensors
and the 8 statistics against the float64 yardstick of tests/deepsets_grad_cases.py, with the method of
tests/test_gpu_trainer.py::test_minibatch_grad_against_the_float64_yardstick -- per tensor err = max|g - g64| / max|g64|, the
bound per case 4 x (torch float32's own error on the same case, measured in the test) + 1e-7, the project's factor for the linear
kernels, for the 19 tensors and for the statistics.  Then determinism and the written-not-accumulated contract, the device-drawn
perturbation, the encoder's share, graph capture, RPOTrainer's wiring and the example.  Everything is compared at the gradient:
nothing after an optimiser step.  The table is printed (run with -s) and copied into DESIGN.md section 4.10."""
import pytest

from tests import deepsets_grad_cases as DC
from tests import encoder_grad_cases as G
from tests.encoder_grad_cases import ea  # noqa: F401  (the fixture)
from tests.test_gpu_trainer import assert_branch_shares, tensor_errors
from tests.trainer_cases import loss_cfg

pytestmark = pytest.mark.gpu
FACTOR = 4


#        N   ed  M      mode       norm_adv clip_vloss ent   alpha
CASES = [(1, 2, 64, "repeat", 0, 1, 0.01, 0.5), (10, 3, 2, "repeat", 1, 1, 0.0, 0.5), (10, 3, 64, "strided", 0, 0, 0.01, 0.0),
         (31, 2, 1000, "strided", 1, 0, 0.0, 0.0), (31, 2, 64, "repeat", 1, 1, 0.01, 0.5), (64, 6, 64, "strided", 0, 0, 0.0, 0.5),
         (64, 6, 1000, "repeat", 0, 1, 0.01, 0.0), (60, 6, 4096, "repeat", 1, 1, 0.01, 0.5), (64, 6, 20000, "strided", 1, 0, 0.0, 0.5)]
BIG = CASES[7]


def case_seed(N, ed, M):
    """(+ 2: with 64 samples and repeated indices the asserted branch shares depend on the draw; settled on the CPU from the
    yardstick alone, before any kernel ran)"""
    return N + ed + M + 2


def test_the_cases_cover_every_axis():
    assert [c[:4] for c in CASES] == [(1, 2, 64, "repeat"), (10, 3, 2, "repeat"), (10, 3, 64, "strided"), (31, 2, 1000, "strided"),
                                      (31, 2, 64, "repeat"), (64, 6, 64, "strided"), (64, 6, 1000, "repeat"), (60, 6, 4096, "repeat"),
                                      (64, 6, 20000, "strided")]
    for ed in (2, 3, 6):
        rows = [c for c in CASES if c[1] == ed]
        assert {c[4] for c in rows} == {0, 1} and {c[5] for c in rows} == {0, 1}
        assert {c[6] for c in rows} == {0.0, 0.01} and {c[7] for c in rows} == {0.0, 0.5}
    assert {(c[4], c[5]) for c in CASES} == {(0, 0), (0, 1), (1, 0), (1, 1)}


ENC = G.Encoder(DC, lambda n: DC.NAMES, tensor_errors, "deepsets_minibatch_grad", "deepsets_kernel_grad", "DeepSetsActorCritic", "deep_sets",
                FACTOR, 13)


@pytest.mark.parametrize("N,ed,M,mode,norm_adv,clip_vloss,ent,alpha", CASES)
def test_minibatch_grad_against_the_float64_yardstick(ea, N, ed, M, mode, norm_adv, clip_vloss, ent, alpha):
    cfg = loss_cfg(norm_adv, clip_vloss, ent, alpha)
    net, batch, inds, z, g64, s64, t = DC.build_case(N, ed, M, mode, cfg, seed=case_seed(N, ed, M))
    assert_branch_shares(t, cfg, M)
    assert 0.2 <= t.relu_on <= 0.8, t.relu_on                                 # at least 20 % of the relu masks are 0, 20 % are 1
    if mode == "repeat" and M >= 64:
        assert int(inds.unique().numel()) < M                                 # indices do repeat
    g32, s32, _ = DC.minibatch_grad(net, batch, inds, cfg, z)                 # torch, float32, on the GPU
    gk, sk = DC.kernel_grad(net, batch, inds, cfg, z)
    assert len(gk) == 19
    G.check_against_float64(ENC, gk, sk, g32, s32, g64, s64,                  # bound (1)
                            f"case N={N} ed={ed} M={M} {mode} norm_adv={norm_adv} clip_vloss={clip_vloss} ent={ent} alpha={alpha}")


def big_case():
    N, ed, M, mode, norm_adv, clip_vloss, ent, alpha = BIG
    cfg = loss_cfg(norm_adv, clip_vloss, ent, alpha)
    return (cfg,) + DC.build_case(N, ed, M, mode, cfg, seed=case_seed(N, ed, M))


def test_deterministic_and_written_not_accumulated(ea):
    G.check_deterministic_and_written_not_accumulated(ENC, *big_case()[:5])


def test_the_encoder_matters(ea):
    import torch
    cfg, net, batch, inds, z, *_ = big_case()
    gk, sk = DC.kernel_grad(net, batch, inds, cfg, z)
    for name, g in zip(DC.ENCODER_NAMES, gk[13:]):
        assert float(g.abs().max()) > 0, name
    sumsq = float(sum((g.double() ** 2).sum() for g in gk))
    assert abs(float(sk[7]) - sumsq) <= 1e-5 * sumsq, (float(sk[7]), sumsq)


def test_in_place_contract_under_graph_capture(ea):
    cfg = loss_cfg(1, 1, 0.01, 0.5)
    G.check_in_place_contract_under_graph_capture(ENC, cfg, *DC.build_case(10, 3, 64, "strided", cfg, seed=21, cache=False)[:4])


def test_trainer_wiring(ea):
    """N = 10, the abs + cat Box observation (D = 36), 8 envs x 16 steps, 2 minibatches x 2 epochs: one update() with
    ``grad_fn = deepsets_kernel_grad``, every call recorded."""
    import torch
    initial, final, _, _ = G.check_trainer_wiring(ENC, ea)
    for name, a, b in zip(DC.NAMES, initial, final):
        assert not torch.equal(a, b), name                                                            # all 19 tensors moved
        assert bool(torch.isfinite(b).all()), name


def test_train_rpo_example_with_the_device_gradient(ea):
    G.check_train_rpo_example_with_the_device_gradient(ENC)
