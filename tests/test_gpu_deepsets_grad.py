"""GPU tests of the deep-sets leader's gradient (evac_deepsets_minibatch_grad, trainer.deepsets_minibatch_grad): all 19 tensors
and the 8 statistics against the float64 yardstick of tests/deepsets_grad_cases.py, with the method of
tests/test_gpu_trainer.py::test_minibatch_grad_against_the_float64_yardstick -- per tensor err = max|g - g64| / max|g64|, the
bound per case 4 x (torch float32's own error on the same case, measured in the test) + 1e-7, the project's factor for the linear
kernels, for the 19 tensors and for the statistics.  Then determinism and the written-not-accumulated contract, the device-drawn
perturbation, the encoder's share, graph capture, RPOTrainer's wiring and the example.  Everything is compared at the gradient:
nothing after an optimiser step.  The table is printed (run with -s) and copied into DESIGN.md section 4.10."""
import math
import os
import subprocess
import sys

import pytest

from tests import deepsets_grad_cases as DC
from tests.test_gpu_trainer import assert_branch_shares, stat_errors, tensor_errors
from tests.trainer_cases import DEV, loss_cfg

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FACTOR = 4


@pytest.fixture(scope="module")
def ea():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("needs an MI355X")
    import evacuation_amd
    return evacuation_amd


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


def check_against_float64(gk, sk, g32, s32, g64, s64, title):
    """Bound (1): every tensor and statistic of the kernel within FACTOR x the float32 yardstick's largest error + 1e-7."""
    e32, ek = tensor_errors(g32, g64), tensor_errors(gk, g64)
    se32, sek = stat_errors(s32, s64), stat_errors(sk, s64)
    bound, sbound = FACTOR * max(e32) + 1e-7, FACTOR * max(se32) + 1e-7
    print(f"\n{title}: e32(case) = {max(e32):.2e}, bound {bound:.2e}; statistics e32 = {max(se32):.2e}, bound {sbound:.2e}")
    for name, a, b in zip(DC.NAMES, e32, ek):
        print(f"  {name:13s} torch f32 {a:.2e}   kernel {b:.2e}   ratio to e32(case) {b / max(e32):.2f}")
    for name, a, b in zip(DC.R.STATS, se32, sek):
        print(f"  {name:13s} torch f32 {a:.2e}   kernel {b:.2e}")
    for name, b in zip(DC.NAMES, ek):
        assert b <= bound, (name, b, bound)
    for name, b in zip(DC.R.STATS, sek):
        assert b <= sbound, (name, b, sbound)


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
    check_against_float64(gk, sk, g32, s32, g64, s64,
                          f"case N={N} ed={ed} M={M} {mode} norm_adv={norm_adv} clip_vloss={clip_vloss} ent={ent} alpha={alpha}")


def big_case():
    N, ed, M, mode, norm_adv, clip_vloss, ent, alpha = BIG
    cfg = loss_cfg(norm_adv, clip_vloss, ent, alpha)
    return (cfg,) + DC.build_case(N, ed, M, mode, cfg, seed=case_seed(N, ed, M))


def test_deterministic_and_written_not_accumulated(ea):
    import torch
    cfg, net, batch, inds, z, *_ = big_case()
    g1, s1 = DC.kernel_grad(net, batch, inds, cfg, z)
    for p in DC.all_tensors(net):
        p.grad.fill_(7.0)                                                     # written, not accumulated
    junk = [torch.randn(1 << 20, device=DEV) for _ in range(5)]               # unrelated allocations and work
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        g2, s2 = DC.kernel_grad(net, batch, inds, cfg, z)
    side.synchronize()
    del junk
    for name, a, b in zip(DC.NAMES, g1, g2):
        assert torch.equal(a, b), name
    assert torch.equal(s1, s2)
    # the perturbation drawn on the device: equal bits for equal (seed, draw_counter), another draw for another counter
    seed, counter = 0x1234567890ABCDEF, (7 << 32) + 5
    gd, sd = DC.kernel_grad(net, batch, inds, cfg, None, seed=seed, draw_counter=counter)
    ge, se = DC.kernel_grad(net, batch, inds, cfg, None, seed=seed, draw_counter=counter)
    for name, a, b in zip(DC.NAMES, gd, ge):
        assert torch.equal(a, b), name
    assert torch.equal(sd, se)
    _, so = DC.kernel_grad(net, batch, inds, cfg, None, seed=seed, draw_counter=counter + 1)
    assert not torch.equal(so, sd)


def test_the_encoder_matters(ea):
    import torch
    cfg, net, batch, inds, z, *_ = big_case()
    gk, sk = DC.kernel_grad(net, batch, inds, cfg, z)
    for name, g in zip(DC.ENCODER_NAMES, gk[13:]):
        assert float(g.abs().max()) > 0, name
    sumsq = float(sum((g.double() ** 2).sum() for g in gk))
    assert abs(float(sk[7]) - sumsq) <= 1e-5 * sumsq, (float(sk[7]), sumsq)


def test_in_place_contract_under_graph_capture(ea):
    import torch
    from evacuation_amd import trainer
    cfg = loss_cfg(1, 1, 0.01, 0.5)
    net, batch, inds, z, *_ = DC.build_case(10, 3, 64, "strided", cfg, seed=21, cache=False)
    stats = torch.zeros(8, device=DEV)
    trainer.deepsets_minibatch_grad(net, batch, inds, cfg, rpo_noise=z, stats=stats)                  # warm-up: binds, allocates
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        trainer.deepsets_minibatch_grad(net, batch, inds, cfg, rpo_noise=z, stats=stats)
    before = [p.grad.clone() for p in DC.all_tensors(net)]
    with torch.no_grad():
        for p in DC.all_tensors(net):
            p.add_(0.05 * torch.randn_like(p))                                                        # in place: same addresses
        inds.copy_(torch.arange(64, device=DEV) * 2)                                                  # other rows, same vector
    graph.replay()
    torch.cuda.synchronize()
    replayed = [p.grad.clone() for p in DC.all_tensors(net)]
    replayed_stats = stats.clone()
    direct, direct_stats = DC.kernel_grad(net, batch, inds, cfg, z)
    for name, a, b, c in zip(DC.NAMES, replayed, direct, before):
        assert torch.equal(a, b), name
        assert not torch.equal(a, c), name
    assert torch.equal(replayed_stats, direct_stats)
    g64, _, _ = DC.minibatch_grad(net, batch, inds, cfg, z, torch.float64)                            # ... and they are the new inputs' gradients
    assert max(tensor_errors(replayed, g64)) < 1e-3


def test_trainer_wiring(ea):
    """N = 10, the abs + cat Box observation (D = 36), 8 envs x 16 steps, 2 minibatches x 2 epochs: one update() with
    ``grad_fn = deepsets_kernel_grad``, every call recorded."""
    import torch
    from evacuation_amd import trainer
    from evacuation_amd.policy import DeepSetsActorCritic
    cfg = trainer.RPOTrainingConfig(seed=3, num_envs=8, num_steps=16, total_timesteps=8 * 16, num_minibatches=2, update_epochs=2)
    env = ea.NormalizedVectorEnv.make(ea.EnvConfig(number_of_pedestrians=10), ea.EnvWrappersConfig(positions="abs", statuses="cat", type="Box"),
                                      num_envs=8, gamma=cfg.gamma, seed=3)
    assert env.obs_dim == 36
    torch.manual_seed(0)
    net = DeepSetsActorCritic(env.obs_dim, 10).to(DEV)
    tensors = DC.all_tensors(net)
    initial = [p.detach().clone() for p in tensors]
    gen = torch.Generator(device=DEV).manual_seed(99)
    calls = []

    def grad_fn(tr, batch, mb_inds, rpo_noise, draw_counter, stats):
        params = [p.detach().clone() for p in tensors]
        out = trainer.deepsets_kernel_grad(tr, batch, mb_inds, rpo_noise, draw_counter, stats)
        calls.append((params, {k: v.clone() for k, v in batch.items()}, mb_inds.clone(), rpo_noise.clone(), draw_counter,
                      [p.grad.clone() for p in tensors], out.clone()))
        return out
    tr = trainer.RPOTrainer(env, net, cfg, grad_fn=grad_fn,
                            rpo_noise_fn=lambda M: (torch.rand(M, 2, device=DEV, generator=gen) * 2 - 1) * cfg.rpo_alpha)
    assert trainer.RPOTrainer(env, net, cfg).grad_fn is trainer.autograd_minibatch_grad           # the default stays autograd's
    log = tr.update()
    torch.cuda.synchronize()
    assert len(calls) == 4 and [c[4] for c in calls] == [0, 1, 2, 3]
    assert all(math.isfinite(v) for k, v in log.items() if isinstance(v, float) and k != "explained_variance"), log
    final = [p.detach().clone() for p in tensors]
    for name, a, b in zip(DC.NAMES, initial, final):
        assert not torch.equal(a, b), name                                                            # all 19 tensors moved
        assert bool(torch.isfinite(b).all()), name
    for i, (params, batch, mb_inds, noise, counter, grads, stats) in enumerate(calls):
        with torch.no_grad():
            for p, q in zip(tensors, params):
                p.copy_(q)                                                                            # the parameters of that moment
        gd, sd = DC.kernel_grad(net, batch, mb_inds, cfg, noise, seed=cfg.seed, draw_counter=counter)
        for name, a, b in zip(DC.NAMES, grads, gd):
            assert torch.equal(a, b), (i, name)
        assert torch.equal(stats, sd)
        g64, s64, _ = DC.minibatch_grad(net, batch, mb_inds, cfg, noise, torch.float64)
        g32, s32, _ = DC.minibatch_grad(net, batch, mb_inds, cfg, noise)
        check_against_float64(grads, stats, g32, s32, g64, s64, f"trainer wiring, call {i}")
    env.close()


def test_train_rpo_example_with_the_device_gradient(ea):
    cmd = [sys.executable, os.path.join(ROOT, "examples", "train_rpo.py"), "--network", "deep_sets", "--gradient", "device", "--envs", "8",
           "--steps", "16", "--updates", "2", "--pedestrians", "10", "--minibatches", "2", "--epochs", "2"]
    done = subprocess.run(cmd, cwd=ROOT, capture_output=True, text=True, timeout=120)
    assert done.returncode == 0, done.stdout[-2000:] + done.stderr[-2000:]
    assert done.stdout.count("SPS:") == 2, done.stdout[-2000:]
