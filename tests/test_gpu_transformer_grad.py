"""GPU tests of the transformer leader's gradient (evac_transformer_minibatch_grad, trainer.transformer_minibatch_grad): all
13 + 16 per block tensors and the 8 statistics against the float64 yardstick of tests/transformer_grad_cases.py, with the method of
tests/test_gpu_deepsets_grad.py -- per tensor err = max|g - g64| / max|g64| (the two key biases, whose exact gradient is zero,
against their weight's largest gradient, a tensor whose float64 gradient vanishes against the case's largest:
transformer_grad_cases.gradient_scales), the bound per case 4 x (torch float32's own largest error on the same case, measured in
the test) + 1e-7, for the tensors and for the statistics.  Then determinism and the written-not-accumulated contract, the
device-drawn perturbation, the sum of squares, the blocks not in use, graph capture, RPOTrainer's wiring and the example.
Everything is compared at the gradient: nothing after an optimiser step.  The table is printed (run with -s) and copied into
DESIGN.md section 4.15."""
import math
import os
import re
import subprocess
import sys

import pytest

from tests import transformer_grad_cases as TC
from tests.test_gpu_trainer import assert_branch_shares, stat_errors
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


def check_against_float64(gk, sk, g32, s32, g64, s64, blocks, title):
    """Every tensor and statistic of the kernel within FACTOR x the float32 yardstick's largest error + 1e-7."""
    e32, ek = TC.tensor_errors(g32, g64, blocks), TC.tensor_errors(gk, g64, blocks)
    se32, sek = stat_errors(s32, s64), stat_errors(sk, s64)
    bound, sbound = FACTOR * max(e32) + 1e-7, FACTOR * max(se32) + 1e-7
    print(f"\n{title}: e32(case) = {max(e32):.2e}, bound {bound:.2e}; statistics e32 = {max(se32):.2e}, bound {sbound:.2e}")
    for name, a, b in zip(TC.names(blocks), e32, ek):
        print(f"  {name:20s} torch f32 {a:.2e}   kernel {b:.2e}   ratio to e32(case) {b / max(e32):.2f}")
    for name, a, b in zip(TC.R.STATS, se32, sek):
        print(f"  {name:20s} torch f32 {a:.2e}   kernel {b:.2e}")
    for name, b in zip(TC.names(blocks), ek):
        assert b <= bound, (name, b, bound)
    for name, b in zip(TC.R.STATS, sek):
        assert b <= sbound, (name, b, sbound)


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
    check_against_float64(gk, sk, g32, s32, g64, s64, blocks,
                          f"case N={N} ed={ed} M={M} blocks={blocks} resid={int(resid)} {mode} norm_adv={norm_adv} "
                          f"clip_vloss={clip_vloss} ent={ent} alpha={alpha}")


def big_case():
    N, ed, M, blocks, resid, mode, norm_adv, clip_vloss, ent, alpha = BIG
    cfg = loss_cfg(norm_adv, clip_vloss, ent, alpha)
    return (cfg,) + TC.build_case(N, ed, M, blocks, resid, mode, cfg, seed=case_seed(N, ed, M))


def test_deterministic_and_written_not_accumulated(ea):
    import torch
    cfg, net, batch, inds, z, *_ = big_case()
    g1, s1 = TC.kernel_grad(net, batch, inds, cfg, z)
    for p in TC.all_tensors(net):
        p.grad.fill_(7.0)                                                     # written, not accumulated
    junk = [torch.randn(1 << 20, device=DEV) for _ in range(5)]               # unrelated allocations and work
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        g2, s2 = TC.kernel_grad(net, batch, inds, cfg, z)
    side.synchronize()
    del junk
    for name, a, b in zip(TC.names(2), g1, g2):
        assert torch.equal(a, b), name
    assert torch.equal(s1, s2)
    # the perturbation drawn on the device: equal bits for equal (seed, draw_counter), another draw for another counter
    seed, counter = 0x1234567890ABCDEF, (7 << 32) + 5
    gd, sd = TC.kernel_grad(net, batch, inds, cfg, None, seed=seed, draw_counter=counter)
    ge, se = TC.kernel_grad(net, batch, inds, cfg, None, seed=seed, draw_counter=counter)
    for name, a, b in zip(TC.names(2), gd, ge):
        assert torch.equal(a, b), name
    assert torch.equal(sd, se)
    _, so = TC.kernel_grad(net, batch, inds, cfg, None, seed=seed, draw_counter=counter + 1)
    assert not torch.equal(so, sd)


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
    enc, enc_grads = st.binder.transformer(net), trainer.ensure_transformer_grads(net)
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
    import torch
    from evacuation_amd import trainer
    cfg = loss_cfg(1, 1, 0.01, 0.5)
    net, batch, inds, z, *_ = TC.build_case(10, 3, 64, 2, False, "strided", cfg, seed=21, cache=False)
    stats = torch.zeros(8, device=DEV)
    trainer.transformer_minibatch_grad(net, batch, inds, cfg, rpo_noise=z, stats=stats)               # warm-up: binds, allocates
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        trainer.transformer_minibatch_grad(net, batch, inds, cfg, rpo_noise=z, stats=stats)
    before = [p.grad.clone() for p in TC.all_tensors(net)]
    with torch.no_grad():
        for p in TC.all_tensors(net):
            p.add_(0.05 * torch.randn_like(p))                                                        # in place: same addresses
        inds.copy_(torch.arange(64, device=DEV) * 2)                                                  # other rows, same vector
    graph.replay()
    torch.cuda.synchronize()
    replayed = [p.grad.clone() for p in TC.all_tensors(net)]
    replayed_stats = stats.clone()
    direct, direct_stats = TC.kernel_grad(net, batch, inds, cfg, z)
    for name, a, b, c in zip(TC.names(2), replayed, direct, before):
        assert torch.equal(a, b), name
        assert not torch.equal(a, c), name
    assert torch.equal(replayed_stats, direct_stats)
    g64, _, _ = TC.minibatch_grad(net, batch, inds, cfg, z, torch.float64)                            # ... and they are the new inputs' gradients
    assert max(TC.tensor_errors(replayed, g64, 2)) < 1e-3


def test_trainer_wiring(ea):
    """N = 10, the abs + cat Box observation (D = 36), 8 envs x 16 steps, 2 minibatches x 2 epochs: one update() with
    ``grad_fn = transformer_kernel_grad``, every call recorded, replayed bit for bit and held to float64."""
    import torch
    from evacuation_amd import trainer
    from evacuation_amd.policy import TransformerActorCritic
    cfg = trainer.RPOTrainingConfig(seed=3, num_envs=8, num_steps=16, total_timesteps=8 * 16, num_minibatches=2, update_epochs=2)
    env = ea.NormalizedVectorEnv.make(ea.EnvConfig(number_of_pedestrians=10), ea.EnvWrappersConfig(positions="abs", statuses="cat", type="Box"),
                                      num_envs=8, gamma=cfg.gamma, seed=3)
    assert env.obs_dim == 36
    torch.manual_seed(0)
    net = TransformerActorCritic(env.obs_dim, 10).to(DEV)
    tensors = TC.all_tensors(net)
    assert len(tensors) == 45
    initial = [p.detach().clone() for p in tensors]
    gen = torch.Generator(device=DEV).manual_seed(99)
    calls = []

    def grad_fn(tr, batch, mb_inds, rpo_noise, draw_counter, stats):
        params = [p.detach().clone() for p in tensors]
        out = trainer.transformer_kernel_grad(tr, batch, mb_inds, rpo_noise, draw_counter, stats)
        calls.append((params, {k: v.clone() for k, v in batch.items()}, mb_inds.clone(), rpo_noise.clone(), draw_counter,
                      [p.grad.clone() for p in tensors], out.clone()))
        return out
    tr = trainer.RPOTrainer(env, net, cfg, grad_fn=grad_fn,
                            rpo_noise_fn=lambda M: (torch.rand(M, 2, device=DEV, generator=gen) * 2 - 1) * cfg.rpo_alpha)
    assert trainer.RPOTrainer(env, net, cfg).grad_fn is trainer.autograd_minibatch_grad           # the default stays autograd's
    with pytest.raises(ValueError, match="`embedding`"):
        trainer.RPOTrainer(env, net, cfg, optimizer="device", grad_fn=trainer.transformer_kernel_grad)
    log = tr.update()
    torch.cuda.synchronize()
    assert len(calls) == 4 and [c[4] for c in calls] == [0, 1, 2, 3]
    assert all(math.isfinite(v) for k, v in log.items() if isinstance(v, float) and k != "explained_variance"), log
    final = [p.detach().clone() for p in tensors]
    assert all(bool(torch.isfinite(b).all()) for b in final)
    assert sum(not torch.equal(a, b) for a, b in zip(initial, final)) >= 43                           # (all but, at most, the two key biases)
    for i, (params, batch, mb_inds, noise, counter, grads, stats) in enumerate(calls):
        with torch.no_grad():
            for p, q in zip(tensors, params):
                p.copy_(q)                                                                            # the parameters of that moment
        gd, sd = TC.kernel_grad(net, batch, mb_inds, cfg, noise, seed=cfg.seed, draw_counter=counter)
        for name, a, b in zip(TC.names(2), grads, gd):
            assert torch.equal(a, b), (i, name)
        assert torch.equal(stats, sd)
        g64, s64, _ = TC.minibatch_grad(net, batch, mb_inds, cfg, noise, torch.float64)
        g32, s32, _ = TC.minibatch_grad(net, batch, mb_inds, cfg, noise)
        check_against_float64(grads, stats, g32, s32, g64, s64, 2, f"trainer wiring, call {i}")
    # what the binder refuses, the entry refuses
    with pytest.raises(ValueError, match="num_heads 2"):
        trainer.transformer_minibatch_grad(TransformerActorCritic(36, 10, num_heads=2).to(DEV), calls[0][1], calls[0][2], cfg)
    env.close()


def test_train_rpo_example_with_the_device_gradient(ea):
    cmd = [sys.executable, os.path.join(ROOT, "examples", "train_rpo.py"), "--network", "transformer", "--gradient", "device", "--envs", "8",
           "--steps", "16", "--updates", "2", "--pedestrians", "10", "--minibatches", "2", "--epochs", "2"]
    done = subprocess.run(cmd, cwd=ROOT, capture_output=True, text=True, timeout=120)
    assert done.returncode == 0, done.stdout[-2000:] + done.stderr[-2000:]
    assert done.stdout.count("SPS:") == 2, done.stdout[-2000:]
