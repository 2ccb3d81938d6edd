"""GPU tests of the deep-sets leader's optimiser step and whole update: evac_deepsets_adam_step bit for bit against the NumPy
statement of its arithmetic over all 19 tensors (tests/optimizer_ref.py), evac_deepsets_minibatch_step == gradient call + step
call, graph capture (the step count lives on the device), evac_deepsets_update == the host loop of minibatch steps including the
early exit at target_kl taken on the device, determinism, RPOTrainer(grad_fn=deepsets_kernel_grad, optimizer="device") and the
example.

Bit for bit means: the float32 / int64 / float64 words are compared as integers."""
import math
import os
import re
import subprocess
import sys
from types import SimpleNamespace

import numpy as np
import pytest

from tests import deepsets_grad_cases as DC
from tests.optimizer_ref import AdamRef
from tests.trainer_cases import DEV, loss_cfg, same_bits

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SCALES = (10.0, 1.0, 1e-3, 1e-5)                 # tests/test_gpu_optimizer.py's: the two large ones clip


@pytest.fixture(scope="module")
def ea():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("needs an MI355X")
    import evacuation_amd
    return evacuation_amd


def twin(N, ed, like, seed=0):
    """A fresh network with the parameters of ``like`` (nothing the library caches on a network is shared, and the cached cases of
    tests/deepsets_grad_cases.py stay as they were built)."""
    import torch
    net = DC.make_net(N, ed, seed=seed)
    with torch.no_grad():
        for p, q in zip(DC.all_tensors(net), DC.all_tensors(like)):
            p.copy_(q)
    return net


def snapshot(net, opt):
    import torch
    torch.cuda.synchronize()
    ts = DC.all_tensors(net)
    assert len(ts) == len(opt.exp_avg) == len(opt.exp_avg_sq) == 19
    return SimpleNamespace(params=[p.detach().clone() for p in ts], grads=[p.grad.detach().clone() for p in ts],
                           m=[t.clone() for t in opt.exp_avg], v=[t.clone() for t in opt.exp_avg_sq], header=opt.read_header())


def assert_same_state(a, b, what):
    for name in ("params", "m", "v", "grads"):
        for i, (x, y) in enumerate(zip(getattr(a, name), getattr(b, name))):
            assert same_bits(x, y), (what, name, DC.NAMES[i], float((x - y).abs().max()))
    for k in ("t", "P1", "P2"):
        assert a.header[k] == b.header[k], (what, k, a.header, b.header)


# ------------------------------------------------------------------------------------------------ evac_deepsets_adam_step
def _random_grads(net, gen, scale):
    import torch
    return [scale * torch.randn(p.shape, generator=gen) for p in DC.all_tensors(net)]


def _step_both(net, opt, ref, ref_params, grads, lr):
    """One step of the kernel and of the yardstick on the same gradients with the same sum of squares; returns the yardstick's
    clipped gradients."""
    import torch
    g_np = [g.numpy().copy() for g in grads]
    sumsq = np.float32(0)
    for g in g_np:
        sumsq = np.float32(sumsq + np.sum(np.square(g, dtype=np.float32), dtype=np.float32))
    with torch.no_grad():
        for p, g in zip(DC.all_tensors(net), grads):
            p.grad.copy_(g)
    opt.param_groups[0]["lr"] = lr
    ref.lr = lr
    opt.step(torch.tensor([sumsq], dtype=torch.float32, device=DEV))
    ref.step(ref_params, g_np, sumsq)
    return g_np


@pytest.mark.parametrize("N,ed", [(1, 2), (10, 3), (64, 6)])
def test_adam_step_is_bit_equal_to_the_yardstick(ea, N, ed):
    """D = 6, 36, 396: the smallest network, a middle one, and the widest, whose 19 tensors span the most workgroups and every
    part-filled tail.  20 consecutive steps from non-zero parameters, gradients of four scales, the learning rate annealed between
    steps: all 19 x {parameter, clipped .grad, exp_avg, exp_avg_sq} and (t, P1, P2) compared after every step."""
    import torch
    from evacuation_amd.trainer import DeviceAdam
    net = DC.make_net(N, ed, seed=N)
    opt = DeviceAdam(net, lr=3e-4, eps=1e-5, max_grad_norm=0.5)
    tensors = DC.all_tensors(net)
    assert len(opt.params) == 19 and int(tensors[0].shape[1]) == (N + 2) * ed
    ref_params = [p.detach().cpu().numpy().copy() for p in tensors]
    assert all(float(np.abs(p).max()) > 0 for p in ref_params[:6] + ref_params[13:17:2])     # (weights; the encoder's too)
    with torch.no_grad():                                                     # non-zero encoder biases too
        for i in (14, 16, 18):
            tensors[i].uniform_(-0.2, 0.2)
    ref_params = [p.detach().cpu().numpy().copy() for p in tensors]
    assert all(float(np.abs(p).max()) > 0 for p in ref_params[13:])
    ref = AdamRef(ref_params, np.float32, lr=3e-4, eps=1e-5, max_grad_norm=0.5)
    gen = torch.Generator().manual_seed(100 + N)
    coefs = []
    for k in range(20):
        g_np = _step_both(net, opt, ref, ref_params, _random_grads(net, gen, SCALES[k % 4]), 3e-4 * (1.0 - k / 20))
        coefs.append(float(ref.last_clip_coef))
        torch.cuda.synchronize()
        for i, (p, rp, rg, m, rm, v, rv) in enumerate(zip(tensors, ref_params, g_np, opt.exp_avg, ref.exp_avg, opt.exp_avg_sq, ref.exp_avg_sq)):
            for name, dev_t, host in (("param", p, rp), ("grad", p.grad, rg), ("exp_avg", m, rm), ("exp_avg_sq", v, rv)):
                got = dev_t.detach().cpu().numpy()
                assert np.array_equal(got.view(np.int32), host.view(np.int32)), \
                    ((N, ed, k), name, DC.NAMES[i], int((got.view(np.int32) != host.view(np.int32)).sum()), float(np.nanmax(np.abs(got - host))))
        h = opt.read_header()
        assert (h["t"], h["P1"], h["P2"]) == (ref.t, ref.P1, ref.P2), (k, h, ref.t, ref.P1, ref.P2)
    assert sum(c == 1.0 for c in coefs) >= 5 and sum(c < 1.0 for c in coefs) >= 5, coefs       # both branches of the clip
    assert opt.step_count == 20


def test_adam_step_keeps_a_nan_from_an_encoder_gradient(ea):
    import torch
    from evacuation_amd.trainer import DeviceAdam
    net = DC.make_net(10, 3, seed=1)
    opt = DeviceAdam(net)
    gen = torch.Generator().manual_seed(5)
    grads = _random_grads(net, gen, 1.0)
    grads[15][3, 4] = float("nan")                                            # phi_w2
    ref_params = [p.detach().cpu().numpy().copy() for p in DC.all_tensors(net)]
    ref = AdamRef(ref_params, np.float32)
    _step_both(net, opt, ref, ref_params, grads, 3e-4)
    torch.cuda.synchronize()
    assert math.isnan(float(ref.last_clip_coef))
    for name, p, m, v in zip(DC.NAMES, DC.all_tensors(net), opt.exp_avg, opt.exp_avg_sq):
        assert bool(torch.isnan(p).all()) and bool(torch.isnan(m).all()) and bool(torch.isnan(v).all()), name
    assert opt.read_header()["t"] == 1


# ------------------------------------------------------------------------------------------------ evac_deepsets_minibatch_step
@pytest.mark.parametrize("N,ed,M", [(1, 2, 2), (10, 3, 64), (64, 6, 300)])
@pytest.mark.parametrize("mode", ["repeat", "strided"])
@pytest.mark.parametrize("norm_adv", [1, 0])
def test_minibatch_step_equals_gradient_then_adam(ea, N, ed, M, mode, norm_adv):
    """Two consecutive steps (the second from non-zero moments): one call against gradient call + step call on a twin network,
    bit for bit: parameters, moments, gradients, statistics, header."""
    from evacuation_amd import trainer
    cfg = loss_cfg(norm_adv, 1, 0.01, 0.5)
    case_net, batch, inds, z, *_ = DC.build_case(N, ed, M, mode, cfg, seed=N + ed + M)
    net_a, net_b = twin(N, ed, case_net), twin(N, ed, case_net)
    opt_a, opt_b = trainer.DeviceAdam(net_a, lr=1e-3), trainer.DeviceAdam(net_b, lr=1e-3)
    start = [p.detach().clone() for p in DC.all_tensors(net_a)]
    for k in range(2):
        stats_a = trainer.deepsets_minibatch_grad(net_a, batch, inds, cfg, rpo_noise=z)
        unclipped = [p.grad.detach().clone() for p in DC.all_tensors(net_a)]
        opt_a.step(stats_a[7])
        stats_b = trainer.deepsets_minibatch_step(net_b, batch, inds, cfg, opt_b, rpo_noise=z)
        a, b = snapshot(net_a, opt_a), snapshot(net_b, opt_b)
        assert_same_state(a, b, (N, ed, M, mode, norm_adv, k))
        assert same_bits(stats_a, stats_b), (stats_a, stats_b)
        assert a.header == b.header and a.header["t"] == k + 1 and a.header["stop"] == 0
        coef = min(1.0, 0.5 / (math.sqrt(float(stats_a[7])) + 1e-6))
        if coef < 0.99:                                                       # .grad holds the CLIPPED gradient, stats[7] the unclipped sum
            assert any(not same_bits(u, g) for u, g in zip(unclipped, b.grads))
    for name, p, q in zip(DC.NAMES, b.params, start):
        assert not same_bits(p, q), name                                      # the steps moved every tensor


def test_captured_step_counts_when_replayed(ea):
    """One deepsets_minibatch_step captured (on the side stream torch.cuda.graph captures on); the minibatch indices and the
    injected noise rewritten in place between replays: 3 replays == 3 direct calls from the same start; the header counts 3."""
    import torch
    from evacuation_amd import trainer
    cfg = loss_cfg(1, 1, 0.01, 0.5)
    N, ed, M = 10, 3, 64
    case_net, batch, inds0, z0, *_ = DC.build_case(N, ed, M, "strided", cfg, seed=21)
    B = batch["b_obs"].shape[0]
    net, direct_net = twin(N, ed, case_net), twin(N, ed, case_net)
    start = [p.detach().clone() for p in DC.all_tensors(net)]
    gen = torch.Generator().manual_seed(3)
    all_inds = [torch.randint(0, B, (M,), generator=gen).to(DEV) for _ in range(3)]
    all_z = [((torch.rand(M, 2, generator=gen) * 2 - 1) * cfg.rpo_alpha).to(DEV) for _ in range(3)]
    inds, z, stats = inds0.clone(), z0.clone(), torch.zeros(8, device=DEV)
    opt = trainer.DeviceAdam(net, lr=1e-3)
    trainer.deepsets_minibatch_step(net, batch, inds, cfg, opt, rpo_noise=z, stats=stats)     # warm-up: binds, allocates ...
    torch.cuda.synchronize()
    with torch.no_grad():                                                                  # ... and is undone, in place
        for p, s in zip(DC.all_tensors(net), start):
            p.copy_(s)
        for t in opt.exp_avg + opt.exp_avg_sq:
            t.zero_()
        opt.header.zero_()
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        trainer.deepsets_minibatch_step(net, batch, inds, cfg, opt, rpo_noise=z, stats=stats)
    replayed_stats = []
    for i in range(3):
        inds.copy_(all_inds[i])
        z.copy_(all_z[i])
        graph.replay()
        replayed_stats.append(stats.clone())
    torch.cuda.synchronize()
    direct_opt = trainer.DeviceAdam(direct_net, lr=1e-3)
    for i in range(3):
        s = trainer.deepsets_minibatch_step(direct_net, batch, all_inds[i], cfg, direct_opt, rpo_noise=all_z[i])
        assert same_bits(s, replayed_stats[i]), i
    a, b = snapshot(net, opt), snapshot(direct_net, direct_opt)
    assert_same_state(a, b, "graph")
    assert a.header["t"] == 3 and a.header["steps_run"] == 3
    assert not same_bits(a.params[0], start[0]) and not same_bits(a.params[13], start[13])


# ------------------------------------------------------------------------------------------------ evac_deepsets_update
def host_loop(trainer, net, batch, perms, cfg, opt, M, noise, seed, first, stats, target_kl=None):
    """The Python loop of minibatch steps that evac_deepsets_update replaces, with the host-side early exit; (steps, epochs)."""
    B = perms.shape[1]
    least = 2 if cfg.norm_adv else 1
    k = epochs = 0
    for e in range(perms.shape[0]):
        last = None
        for start in range(0, B, M):
            inds = perms[e, start:start + M]
            m = int(inds.shape[0])
            if m < least:
                continue
            last = trainer.deepsets_minibatch_step(net, batch, inds, cfg, opt, rpo_noise=None if noise is None else noise[k, :m], seed=seed,
                                                   draw_counter=first + k, stats=stats[k])
            k += 1
        epochs += 1
        if target_kl is not None and float(last[5]) > target_kl:
            break
    return k, epochs


def _update_case(N, ed, B, norm_adv, seed, alpha=0.5):
    cfg = loss_cfg(norm_adv, 1, 0.01, alpha)
    net, batch, *_ = DC.build_case(N, ed, B, "repeat", cfg, seed=seed)
    assert batch["b_obs"].shape[0] == B
    return cfg, net, batch


UPDATE_CASES = [  # N, ed, B, M, norm_adv, injected noise, steps per epoch
    (10, 3, 256, 64, 1, False, 4),            # B a multiple of M
    (10, 3, 200, 64, 1, False, 4),            # a tail of 8 that runs
    (10, 3, 193, 64, 1, False, 3),            # a tail of 1 with norm_adv: skipped
    (10, 3, 193, 64, 0, False, 4),            # ... and runs without it
    (64, 6, 128, 64, 1, True, 2)]             # the widest network, injected noise


@pytest.mark.parametrize("N,ed,B,M,norm_adv,inject,per_epoch", UPDATE_CASES)
def test_update_equals_the_host_loop(ea, N, ed, B, M, norm_adv, inject, per_epoch):
    import torch
    from evacuation_amd import trainer
    cfg, case_net, batch = _update_case(N, ed, B, norm_adv, seed=40 + N + B)
    net_a, net_b = twin(N, ed, case_net), twin(N, ed, case_net)
    assert len(trainer.update_steps(B, M, bool(norm_adv))) == per_epoch
    steps = 3 * per_epoch
    gen = torch.Generator().manual_seed(B)
    perms = torch.stack([torch.randperm(B, generator=gen) for _ in range(3)]).to(DEV)
    noise = ((torch.rand(steps, M, 2, generator=gen) * 2 - 1) * cfg.rpo_alpha).to(DEV).contiguous() if inject else None
    opt_a, opt_b = trainer.DeviceAdam(net_a, lr=1e-3), trainer.DeviceAdam(net_b, lr=1e-3)
    stats_a = torch.full((steps, 8), -7.0, device=DEV)
    stats_b = torch.full((steps, 8), -7.0, device=DEV)
    out, header = trainer.deepsets_update(net_a, batch, perms, cfg, opt_a, rpo_noise=noise, seed=11, first_draw_counter=1000, stats=stats_a,
                                          minibatch_size=M)
    assert out is stats_a
    ran, epochs = host_loop(trainer, net_b, batch, perms, cfg, opt_b, M, noise, 11, 1000, stats_b)
    a, b = snapshot(net_a, opt_a), snapshot(net_b, opt_b)
    assert (ran, epochs) == (steps, 3)
    h = trainer.decode_header(header)
    assert (h["steps_run"], h["epochs_run"], h["stop"], h["t"]) == (steps, 3, 0, steps), h
    assert_same_state(a, b, (N, ed, B, M))
    assert same_bits(stats_a, stats_b)
    assert not bool((stats_a == -7.0).any())


def _own_logprobs_case():
    """tests/test_gpu_optimizer.py::test_target_kl_is_taken_on_the_device's construction: old log-probabilities that are the
    network's own and no RPO perturbation, so approx_kl starts at zero and grows as the policy moves."""
    import torch
    N, ed, B = 10, 3, 256
    cfg, case_net, batch = _update_case(N, ed, B, 1, seed=77, alpha=0.0)
    batch = dict(batch)
    with torch.no_grad():
        _, lp, _, _ = case_net.get_action_and_value(batch["b_obs"], batch["b_actions"])
        batch["b_logprobs"] = lp.contiguous()
    return N, ed, B, cfg, case_net, batch


def test_target_kl_is_taken_on_the_device(ea):
    """The early exit of rpo_agent.py:281-283 without the host.  The learning rate is the reference's default, 3e-4: this
    network's actor head is 40 times the initial one (tests/deepsets_grad_cases.make_net), and at the linear test's 1e-3 the
    policy of 64-sample minibatches has moved furthest by the end of the FIRST epoch, after which the closing approx_kl never
    exceeds that value again and there is no epoch to stop at."""
    import torch
    from evacuation_amd import trainer
    N, ed, B, cfg, net0, batch = _own_logprobs_case()
    M, n_epochs, lr = 64, 5, 3e-4
    gen = torch.Generator().manual_seed(8)
    perms = torch.stack([torch.randperm(B, generator=gen) for _ in range(n_epochs)]).to(DEV)
    steps = n_epochs * (B // M)

    def fresh():
        net = twin(N, ed, net0)
        return net, trainer.DeviceAdam(net, lr=lr)

    # 1. the host-driven loop without a target: every epoch's closing approx_kl
    net, opt = fresh()
    stats = torch.zeros(steps, 8, device=DEV)
    assert host_loop(trainer, net, batch, perms, cfg, opt, M, None, 5, 0, stats) == (steps, n_epochs)
    closing = [float(stats[(e + 1) * (B // M) - 1, 5]) for e in range(n_epochs)]
    print("\nclosing approx_kl per epoch:", " ".join(f"{x:.3e}" for x in closing))
    star = next((e for e in range(1, n_epochs - 1) if closing[e] > max(closing[:e])), None)
    assert n_epochs >= 4 and star is not None, closing                            # (fails, not skips)
    cfg.target_kl = 0.5 * (closing[star] + max(closing[:star]))
    try:
        # 2. the host-driven loop that breaks at that epoch
        net_h, opt_h = fresh()
        stats_h = torch.full((steps, 8), -7.0, device=DEV)
        ran_h, epochs_h = host_loop(trainer, net_h, batch, perms, cfg, opt_h, M, None, 5, 0, stats_h, target_kl=cfg.target_kl)
        assert epochs_h == star + 1 and ran_h == (star + 1) * (B // M)
        # 3. one call
        net_d, opt_d = fresh()
        stats_d = torch.full((steps, 8), -7.0, device=DEV)
        _, header = trainer.deepsets_update(net_d, batch, perms, cfg, opt_d, seed=5, first_draw_counter=0, stats=stats_d, minibatch_size=M)
        a, b = snapshot(net_d, opt_d), snapshot(net_h, opt_h)
        h = trainer.decode_header(header)
        assert (h["epochs_run"], h["steps_run"], h["stop"], h["t"]) == (star + 1, ran_h, 1, ran_h), h
        assert_same_state(a, b, "target_kl")
        assert same_bits(stats_d, stats_h)
        assert bool((stats_d[ran_h:] == -7.0).all()) and not bool((stats_d[:ran_h] == -7.0).any())
    finally:
        cfg.target_kl = None
    # a later call clears the flag and runs
    trainer.deepsets_update(net_d, batch, perms[:1].contiguous(), cfg, opt_d, seed=5, stats=stats_d[:B // M], minibatch_size=M)
    h = opt_d.read_header()
    assert (h["stop"], h["steps_run"], h["epochs_run"], h["t"]) == (0, B // M, 1, ran_h + B // M), h


def test_the_same_update_twice_gives_the_same_bits(ea):
    """Determinism of the whole step: deepsets_update (drawn perturbations) twice from the same start on twin networks."""
    import torch
    from evacuation_amd import trainer
    N, ed, B, M = 10, 3, 200, 64
    cfg, case_net, batch = _update_case(N, ed, B, 1, seed=40 + N + B)
    gen = torch.Generator().manual_seed(2)
    perms = torch.stack([torch.randperm(B, generator=gen) for _ in range(2)]).to(DEV)
    out = []
    for _ in range(2):
        net = twin(N, ed, case_net)
        opt = trainer.DeviceAdam(net, lr=1e-3)
        stats, _ = trainer.deepsets_update(net, batch, perms, cfg, opt, seed=9, first_draw_counter=3, minibatch_size=M)
        out.append((snapshot(net, opt), stats.clone()))
    assert_same_state(out[0][0], out[1][0], "twice")
    assert out[0][0].header == out[1][0].header and out[0][0].header["t"] == 8
    assert same_bits(out[0][1], out[1][1])


# ------------------------------------------------------------------------------------------------ RPOTrainer
LOGGED = ("loss", "value_loss", "policy_loss", "entropy", "old_approx_kl", "approx_kl", "learning_rate")


def _make_trainer(ea, **hooks):
    import torch
    from evacuation_amd import trainer
    from evacuation_amd.policy import DeepSetsActorCritic
    cfg = trainer.RPOTrainingConfig(seed=3, num_envs=16, num_steps=32, total_timesteps=16 * 32 * 2, num_minibatches=4, update_epochs=2)
    env = ea.NormalizedVectorEnv.make(ea.EnvConfig(number_of_pedestrians=10), ea.EnvWrappersConfig(positions="rel", statuses="ohe", type="Box"),
                                      num_envs=16, gamma=cfg.gamma, seed=3)
    torch.manual_seed(0)
    net = DeepSetsActorCritic(env.obs_dim, 10).to(DEV)
    return trainer.RPOTrainer(env, net, cfg, **hooks)


def test_trainer_with_the_device_optimiser(ea):
    """N = 10, the rel + ohe Box observation, 16 envs x 32 steps, 4 minibatches x 2 epochs, two update()s: one deepsets_update
    per update and one deepsets_minibatch_step per minibatch on twin handles are bit-equal after each update."""
    import torch
    from evacuation_amd import trainer
    one = _make_trainer(ea, grad_fn=trainer.deepsets_kernel_grad, optimizer="device", one_call=True)
    per = _make_trainer(ea, grad_fn=trainer.deepsets_kernel_grad, optimizer="device", one_call=False)
    initial = [p.detach().clone() for p in DC.all_tensors(one.net)]
    logged = 0
    for u in range(2):
        la, lb = one.update(), per.update()
        a, b = snapshot(one.net, one.optimizer), snapshot(per.net, per.optimizer)
        assert_same_state(a, b, ("trainer", u))
        assert set(la) == set(lb)
        for k in LOGGED:
            assert la[k] == lb[k] and math.isfinite(la[k]), (u, k, la[k], lb[k])
        assert abs(la["clipfrac"] - lb["clipfrac"]) <= 1e-6
        logged += 2 * 4
        assert one.minibatch_steps == per.minibatch_steps == logged
    assert one.optimizer.step_count == per.optimizer.step_count == logged == 16
    for name, p, q in zip(DC.NAMES, DC.all_tensors(one.net), initial):
        assert not torch.equal(p.detach(), q) and bool(torch.isfinite(p).all()), name      # all 19 tensors moved
    one.env.close()
    per.env.close()
    # any other grad_fn is followed by the optimiser's own step
    auto = _make_trainer(ea, grad_fn=trainer.autograd_minibatch_grad, optimizer="device")
    before = [p.detach().clone() for p in DC.all_tensors(auto.net)]
    log = auto.update()
    torch.cuda.synchronize()
    assert math.isfinite(log["loss"]) and auto.optimizer.step_count == 8 and auto.minibatch_steps == 8
    for name, p, q in zip(DC.NAMES, DC.all_tensors(auto.net), before):
        assert not torch.equal(p.detach(), q) and bool(torch.isfinite(p).all()), name
    # the default gradient of such a network is autograd's: with it the device optimiser stays refused
    with pytest.raises(ValueError, match="gradient and optimiser kernels are the linear network's"):
        trainer.RPOTrainer(auto.env, auto.net, auto.cfg, optimizer="device")
    auto.env.close()


def test_train_rpo_example_with_the_device_optimiser(ea):
    cmd = [sys.executable, os.path.join(ROOT, "examples", "train_rpo.py"), "--network", "deep_sets", "--gradient", "device", "--optimizer",
           "device", "--envs", "8", "--steps", "16", "--updates", "2", "--pedestrians", "10", "--minibatches", "2", "--epochs", "2"]
    done = subprocess.run(cmd, cwd=ROOT, capture_output=True, text=True, timeout=120)
    assert done.returncode == 0, done.stdout[-2000:] + done.stderr[-2000:]
    assert done.stdout.count("SPS:") == 2, done.stdout[-2000:]
    losses = re.findall(r"value_loss=(\S+)\s+policy_loss=(\S+)\s+approx_kl=(\S+)", done.stdout)
    assert len(losses) == 2 and all(math.isfinite(float(x)) for row in losses for x in row), done.stdout[-2000:]
