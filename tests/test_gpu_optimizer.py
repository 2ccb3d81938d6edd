"""GPU tests of the optimiser step on the device: evac_adam_step bit for bit against the NumPy statement of its arithmetic
(tests/optimizer_ref.py), evac_rpo_minibatch_step == gradient call + step call, accuracy over a short run with a tolerance measured
from torch's own float32 error, graph capture (the step count lives on the device), evac_rpo_update == the host loop of minibatch
steps including the early exit at target_kl taken on the device, DeviceAdam's state dict, and RPOTrainer(optimizer="device").

Bit for bit means: the float32 / int64 / float64 words are compared as integers."""
import math
from types import SimpleNamespace

import numpy as np
import pytest

from tests import trainer_ref as R
from tests.optimizer_ref import AdamRef
from tests.trainer_cases import DEV, _yardstick_grad_fn, build_case, loss_cfg, make_initial_net, make_net, make_trainer, same_bits

pytestmark = pytest.mark.gpu
SCALES = (10.0, 1.0, 1e-3, 1e-5)


@pytest.fixture(scope="module")
def ea():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("needs an MI355X")
    import evacuation_amd
    return evacuation_amd


def twin(net_seed, D, like):
    """A second network with the parameters of ``like`` (a fresh module: nothing the library caches on a network is shared)."""
    import torch
    net = make_net(D, seed=net_seed)
    with torch.no_grad():
        for p, q in zip(R.mlp_tensors(net), R.mlp_tensors(like)):
            p.copy_(q)
    return net


def snapshot(net, opt):
    import torch
    torch.cuda.synchronize()
    return SimpleNamespace(params=[p.detach().clone() for p in R.mlp_tensors(net)], grads=[p.grad.detach().clone() for p in R.mlp_tensors(net)],
                           m=[t.clone() for t in opt.exp_avg], v=[t.clone() for t in opt.exp_avg_sq], header=opt.read_header())


def assert_same_state(a, b, what, grads=True):
    for name in ("params", "m", "v") + (("grads",) if grads else ()):
        for i, (x, y) in enumerate(zip(getattr(a, name), getattr(b, name))):
            assert same_bits(x, y), (what, name, R.NAMES[i], float((x - y).abs().max()))
    for k in ("t", "P1", "P2"):
        assert a.header[k] == b.header[k], (what, k, a.header, b.header)


# ------------------------------------------------------------------------------------------------ evac_adam_step
def _random_grads(net, gen, scale):
    import torch
    return [scale * torch.randn(p.shape, generator=gen) for p in R.mlp_tensors(net)]


def _step_both(net, opt, ref, ref_params, grads, lr):
    """One step of the kernel and of the yardstick on the same gradients with the same sum of squares; returns the yardstick's
    clipped gradients."""
    import torch
    g_np = [g.numpy().copy() for g in grads]
    sumsq = np.float32(0)
    for g in g_np:
        sumsq = np.float32(sumsq + np.sum(np.square(g, dtype=np.float32), dtype=np.float32))
    with torch.no_grad():
        for p, g in zip(R.mlp_tensors(net), grads):
            p.grad.copy_(g)
    opt.param_groups[0]["lr"] = lr
    ref.lr = lr
    opt.step(torch.tensor([sumsq], dtype=torch.float32, device=DEV))
    ref.step(ref_params, g_np, sumsq)
    return g_np


def _assert_equals_ref(net, opt, ref, ref_params, g_np, what):
    import torch
    torch.cuda.synchronize()
    for i, (p, rp, rg, m, rm, v, rv) in enumerate(zip(R.mlp_tensors(net), ref_params, g_np, opt.exp_avg, ref.exp_avg, opt.exp_avg_sq, ref.exp_avg_sq)):
        for name, dev_t, host in (("param", p, rp), ("grad", p.grad, rg), ("exp_avg", m, rm), ("exp_avg_sq", v, rv)):
            got = dev_t.detach().cpu().numpy()
            assert np.array_equal(got.view(np.int32), host.view(np.int32)), \
                (what, name, R.NAMES[i], int((got.view(np.int32) != host.view(np.int32)).sum()), float(np.nanmax(np.abs(got - host))))
    h = opt.read_header()
    assert (h["t"], h["P1"], h["P2"]) == (ref.t, ref.P1, ref.P2), (what, h, ref.t, ref.P1, ref.P2)


@pytest.mark.parametrize("D", [6, 124, 396])
def test_adam_step_is_bit_equal_to_the_yardstick(ea, D):
    """50 consecutive steps from non-zero parameters, gradients of four scales (the two large ones clip), the learning rate
    annealed between steps: parameters, both moments, the clipped .grad and the header compared after every step."""
    import torch
    from evacuation_amd.trainer import DeviceAdam
    net = make_net(D, seed=D)
    opt = DeviceAdam(net, lr=3e-4, eps=1e-5, max_grad_norm=0.5)
    ref_params = [p.detach().cpu().numpy().copy() for p in R.mlp_tensors(net)]
    assert all(float(np.abs(p).max()) > 0 for p in ref_params[:6])
    ref = AdamRef(ref_params, np.float32, lr=3e-4, eps=1e-5, max_grad_norm=0.5)
    gen = torch.Generator().manual_seed(100 + D)
    coefs = []
    for k in range(50):
        g_np = _step_both(net, opt, ref, ref_params, _random_grads(net, gen, SCALES[k % 4]), 3e-4 * (1.0 - k / 50))
        coefs.append(float(ref.last_clip_coef))
        _assert_equals_ref(net, opt, ref, ref_params, g_np, (D, k))
    assert sum(c == 1.0 for c in coefs) >= 20 and sum(c < 1.0 for c in coefs) >= 20, coefs       # both branches of the clip
    assert opt.step_count == 50


def test_adam_step_keeps_a_nan(ea):
    """A NaN in the gradients makes their sum of squares a NaN: every parameter comes out NaN, as under clip_grad_norm_ with its
    default error_if_nonfinite=False."""
    import torch
    from evacuation_amd.trainer import DeviceAdam
    net = make_net(6, seed=1)
    opt = DeviceAdam(net)
    gen = torch.Generator().manual_seed(5)
    grads = _random_grads(net, gen, 1.0)
    grads[2][3, 4] = float("nan")
    ref_params = [p.detach().cpu().numpy().copy() for p in R.mlp_tensors(net)]
    ref = AdamRef(ref_params, np.float32)
    _step_both(net, opt, ref, ref_params, grads, 3e-4)
    torch.cuda.synchronize()
    assert math.isnan(float(ref.last_clip_coef))
    for p, rp, m, v in zip(R.mlp_tensors(net), ref_params, opt.exp_avg, opt.exp_avg_sq):
        assert bool(torch.isnan(p).all()) and np.isnan(rp).all()
        assert bool(torch.isnan(p.grad).all()) and bool(torch.isnan(m).all()) and bool(torch.isnan(v).all())
    assert opt.read_header()["t"] == 1


# ------------------------------------------------------------------------------------------------ evac_rpo_minibatch_step
@pytest.mark.parametrize("D", [6, 396])
@pytest.mark.parametrize("M", [2, 64, 16384])
@pytest.mark.parametrize("mode", ["repeat", "strided"])
def test_minibatch_step_equals_gradient_then_adam(ea, D, M, mode):
    """Two consecutive steps (the second from non-zero moments): one call against gradient call + step call, bit for bit; the
    statistics are those of the gradient at the parameters before the step."""
    import torch
    from evacuation_amd import trainer
    cfg = loss_cfg(1, 1, 0.01, 0.5)
    seed = D + M
    net_a, batch, inds, z, *_ = build_case(D, M, mode, cfg, seed=seed)
    net_b = twin(seed, D, net_a)
    opt_a, opt_b = trainer.DeviceAdam(net_a, lr=1e-3), trainer.DeviceAdam(net_b, lr=1e-3)
    start = [p.detach().clone() for p in R.mlp_tensors(net_a)]
    for k in range(2):
        stats_a = trainer.rpo_minibatch_grad(net_a, batch, inds, cfg, rpo_noise=z)
        unclipped = [p.grad.detach().clone() for p in R.mlp_tensors(net_a)]
        opt_a.step(stats_a[7])
        stats_b = trainer.rpo_minibatch_step(net_b, batch, inds, cfg, opt_b, rpo_noise=z)
        a, b = snapshot(net_a, opt_a), snapshot(net_b, opt_b)
        assert_same_state(a, b, (D, M, mode, k))
        assert same_bits(stats_a, stats_b), (stats_a, stats_b)
        assert a.header["t"] == k + 1
        coef = min(1.0, 0.5 / (math.sqrt(float(stats_a[7])) + 1e-6))
        if coef < 0.99:                                                           # .grad holds the CLIPPED gradient, stats[7] the unclipped sum
            assert any(not same_bits(u, g) for u, g in zip(unclipped, b.grads))
        assert any(not same_bits(p, q) for p, q in zip(b.params, start))             # the step moved the parameters


# ------------------------------------------------------------------------------------------------ accuracy over a short run
def _torch_driven(net, batch, perms, noise, cfg, M, dtype, lr):
    """K minibatch steps with the yardstick's loss, autograd, clip_grad_norm_ and Adam(eps=1e-5) in ``dtype`` on the GPU."""
    import torch
    P = R.params_of(net, dtype)
    opt = torch.optim.Adam(P, lr=lr, eps=1e-5)
    b = {k: v.to(dtype) for k, v in batch.items()}
    k = 0
    for e in range(perms.shape[0]):
        for start in range(0, perms.shape[1], M):
            t = R.loss_terms(P, b, perms[e, start:start + M], cfg, noise[k].to(dtype))
            opt.zero_grad()
            t.loss.backward()
            torch.nn.utils.clip_grad_norm_(P, 0.5)
            opt.step()
            k += 1
    return [p.detach().double() for p in P]


@pytest.mark.parametrize("D,norm_adv,clip_vloss", [(6, 1, 1), (6, 0, 0), (124, 1, 0), (396, 1, 1)])
def test_accuracy_over_sixteen_steps(ea, D, norm_adv, clip_vloss):
    """K = 16 consecutive minibatch steps (4 epochs x 4 minibatches of 1024 of one batch of 4096) three ways from one start:
    float64 master, torch float32, the kernels.  e32 = max |float32-driven - float64-driven| over the parameters, ek likewise for
    the kernels: ek <= 4 x e32 + 1e-7.  Short on purpose: the loss has kinks, and a sample that crosses one in one arithmetic
    and not in the other separates two runs by more than rounding."""
    import torch
    from evacuation_amd import trainer
    cfg = loss_cfg(norm_adv, clip_vloss, 0.01, 0.5)
    B, M, lr = 4096, 1024, 3e-4
    net, batch, *_ = build_case(D, B, "repeat", cfg, seed=300 + D)
    gen = torch.Generator().manual_seed(17)
    perms = torch.stack([torch.randperm(B, generator=gen) for _ in range(4)]).to(DEV)
    noise = ((torch.rand(16, M, 2, generator=gen) * 2 - 1) * cfg.rpo_alpha).to(DEV).contiguous()
    p64 = _torch_driven(net, batch, perms, noise, cfg, M, torch.float64, lr)
    p32 = _torch_driven(net, batch, perms, noise, cfg, M, torch.float32, lr)
    start = [p.detach().double().clone() for p in R.mlp_tensors(net)]
    opt = trainer.DeviceAdam(net, lr=lr, eps=1e-5, max_grad_norm=0.5)
    k = 0
    for e in range(4):
        for s in range(0, B, M):
            trainer.rpo_minibatch_step(net, batch, perms[e, s:s + M], cfg, opt, rpo_noise=noise[k])
            k += 1
    torch.cuda.synchronize()
    pk = [p.detach().double() for p in R.mlp_tensors(net)]
    e32 = max(float((x - y).abs().max()) for x, y in zip(p32, p64))
    ek = max(float((x - y).abs().max()) for x, y in zip(pk, p64))
    moved = max(float((x - y).abs().max()) for x, y in zip(p64, start))
    print(f"\n16 steps D={D} norm_adv={norm_adv} clip_vloss={clip_vloss}: e32 = {e32:.3e}, ek = {ek:.3e}, bound {4 * e32 + 1e-7:.3e}; "
          f"the parameters moved by {moved:.3e}")
    assert moved > 1e-3 and opt.step_count == 16
    assert ek <= 4 * e32 + 1e-7, (ek, e32)


# ------------------------------------------------------------------------------------------------ graph capture
def test_captured_step_counts_when_replayed(ea):
    """One rpo_minibatch_step captured; the minibatch indices and the injected noise rewritten in place between replays:
    5 replays == 5 direct calls with the same arguments from the same start, and the header counts 5 steps."""
    import torch
    from evacuation_amd import trainer
    cfg = loss_cfg(1, 1, 0.01, 0.5)
    D, M = 6, 1000
    net, batch, inds0, z0, *_ = build_case(D, M, "strided", cfg, seed=21)
    B = batch["b_obs"].shape[0]
    direct_net = twin(21, D, net)
    start = [p.detach().clone() for p in R.mlp_tensors(net)]
    gen = torch.Generator().manual_seed(3)
    all_inds = [torch.randint(0, B, (M,), generator=gen).to(DEV) for _ in range(5)]
    all_z = [((torch.rand(M, 2, generator=gen) * 2 - 1) * cfg.rpo_alpha).to(DEV) for _ in range(5)]
    inds, z, stats = inds0.clone(), z0.clone(), torch.zeros(8, device=DEV)
    opt = trainer.DeviceAdam(net, lr=1e-3)
    trainer.rpo_minibatch_step(net, batch, inds, cfg, opt, rpo_noise=z, stats=stats)          # warm-up: binds, allocates ...
    torch.cuda.synchronize()
    with torch.no_grad():                                                                  # ... and is undone, in place
        for p, s in zip(R.mlp_tensors(net), start):
            p.copy_(s)
        for t in opt.exp_avg + opt.exp_avg_sq:
            t.zero_()
        opt.header.zero_()
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        trainer.rpo_minibatch_step(net, batch, inds, cfg, opt, rpo_noise=z, stats=stats)
    replayed_stats = []
    for i in range(5):
        inds.copy_(all_inds[i])
        z.copy_(all_z[i])
        graph.replay()
        replayed_stats.append(stats.clone())
    torch.cuda.synchronize()
    direct_opt = trainer.DeviceAdam(direct_net, lr=1e-3)
    for i in range(5):
        s = trainer.rpo_minibatch_step(direct_net, batch, all_inds[i], cfg, direct_opt, rpo_noise=all_z[i])
        assert same_bits(s, replayed_stats[i]), i
    a, b = snapshot(net, opt), snapshot(direct_net, direct_opt)
    assert_same_state(a, b, "graph")
    assert a.header["t"] == 5 and a.header["steps_run"] == 5
    assert not same_bits(a.params[0], start[0])


# ------------------------------------------------------------------------------------------------ evac_rpo_update
def host_loop(trainer, net, batch, perms, cfg, opt, M, noise, seed, first, stats, target_kl=None):
    """The Python loop of minibatch steps that evac_rpo_update replaces, with the host-side early exit; returns (steps, epochs)."""
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
            last = trainer.rpo_minibatch_step(net, batch, inds, cfg, opt, rpo_noise=None if noise is None else noise[k, :m], seed=seed,
                                              draw_counter=first + k, stats=stats[k])
            k += 1
        epochs += 1
        if target_kl is not None and float(last[5]) > target_kl:
            break
    return k, epochs


def _update_case(D, B, norm_adv, seed, alpha=0.5):
    import torch
    cfg = loss_cfg(norm_adv, 1, 0.01, alpha)
    net, batch, *_ = build_case(D, B, "repeat", cfg, seed=seed)
    assert batch["b_obs"].shape[0] == B
    return cfg, net, batch


UPDATE_CASES = [  # D, B, M, norm_adv, injected noise, steps per epoch
    (6, 1024, 256, 1, False, 4), (6, 1024, 256, 1, True, 4),          # B a multiple of M
    (6, 1000, 256, 1, False, 4), (396, 1000, 256, 0, True, 4),        # B mod M = 232: the tail runs
    (6, 1025, 256, 1, True, 4), (6, 1025, 256, 1, False, 4),          # B mod M = 1 with norm_adv: the tail is skipped
    (6, 1025, 256, 0, False, 5)]                                       # ... and runs without it


@pytest.mark.parametrize("D,B,M,norm_adv,inject,per_epoch", UPDATE_CASES)
def test_update_equals_the_host_loop(ea, D, B, M, norm_adv, inject, per_epoch):
    import torch
    from evacuation_amd import trainer
    cfg, net_a, batch = _update_case(D, B, norm_adv, seed=40 + D + B)
    net_b = twin(40 + D + B, D, net_a)
    assert trainer.update_steps(B, M, bool(norm_adv)) == [M] * (B // M) + ([B % M] if per_epoch > B // M else [])
    steps = 3 * per_epoch
    gen = torch.Generator().manual_seed(B)
    perms = torch.stack([torch.randperm(B, generator=gen) for _ in range(3)]).to(DEV)
    noise = ((torch.rand(steps, M, 2, generator=gen) * 2 - 1) * cfg.rpo_alpha).to(DEV).contiguous() if inject else None
    opt_a, opt_b = trainer.DeviceAdam(net_a, lr=1e-3), trainer.DeviceAdam(net_b, lr=1e-3)
    stats_a = torch.full((steps, 8), -7.0, device=DEV)
    stats_b = torch.full((steps, 8), -7.0, device=DEV)
    out, header = trainer.rpo_update(net_a, batch, perms, cfg, opt_a, rpo_noise=noise, seed=11, first_draw_counter=1000, stats=stats_a,
                                     minibatch_size=M)
    assert out is stats_a
    ran, epochs = host_loop(trainer, net_b, batch, perms, cfg, opt_b, M, noise, 11, 1000, stats_b)
    a, b = snapshot(net_a, opt_a), snapshot(net_b, opt_b)
    assert (ran, epochs) == (steps, 3)
    h = trainer.decode_header(header)
    assert (h["steps_run"], h["epochs_run"], h["stop"], h["t"]) == (steps, 3, 0, steps), h
    assert_same_state(a, b, (D, B, M))
    assert same_bits(stats_a, stats_b)
    assert not bool((stats_a == -7.0).any())


def test_target_kl_is_taken_on_the_device(ea):
    """The early exit of rpo_agent.py:281-283 without the host.  The case (chosen on the host-driven loop): a batch whose old
    log-probabilities are the network's own and no RPO perturbation, so approx_kl starts at zero and grows as the policy moves."""
    import torch
    from evacuation_amd import trainer
    D, B, M, n_epochs, lr = 6, 1024, 256, 5, 1e-3
    cfg, net0, batch = _update_case(D, B, 1, seed=77, alpha=0.0)
    with torch.no_grad():
        P = [p.detach() for p in R.mlp_tensors(net0)]
        lp, _, _ = R.logprob_entropy_value(P, batch["b_obs"], batch["b_actions"], torch.zeros(B, 2, device=DEV))
        batch["b_logprobs"] = lp.contiguous()
    gen = torch.Generator().manual_seed(8)
    perms = torch.stack([torch.randperm(B, generator=gen) for _ in range(n_epochs)]).to(DEV)
    steps = n_epochs * (B // M)

    def fresh():
        net = twin(77, D, net0)
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
    # 2. the host-driven loop that breaks at that epoch
    net_h, opt_h = fresh()
    stats_h = torch.full((steps, 8), -7.0, device=DEV)
    ran_h, epochs_h = host_loop(trainer, net_h, batch, perms, cfg, opt_h, M, None, 5, 0, stats_h, target_kl=cfg.target_kl)
    assert epochs_h == star + 1 and ran_h == (star + 1) * (B // M)
    # 3. one call
    net_d, opt_d = fresh()
    stats_d = torch.full((steps, 8), -7.0, device=DEV)
    _, header = trainer.rpo_update(net_d, batch, perms, cfg, opt_d, seed=5, first_draw_counter=0, stats=stats_d, minibatch_size=M)
    a, b = snapshot(net_d, opt_d), snapshot(net_h, opt_h)
    h = trainer.decode_header(header)
    assert (h["epochs_run"], h["steps_run"], h["stop"], h["t"]) == (star + 1, ran_h, 1, ran_h), h
    assert_same_state(a, b, "target_kl")
    assert same_bits(stats_d, stats_h)
    assert bool((stats_d[ran_h:] == -7.0).all()) and not bool((stats_d[:ran_h] == -7.0).any())
    # a later call clears the flag and runs
    cfg.target_kl = None
    trainer.rpo_update(net_d, batch, perms[:1].contiguous(), cfg, opt_d, seed=5, stats=stats_d[:B // M], minibatch_size=M)
    h = opt_d.read_header()
    assert (h["stop"], h["steps_run"], h["epochs_run"], h["t"]) == (0, B // M, 1, ran_h + B // M), h


# ------------------------------------------------------------------------------------------------ DeviceAdam's state dict
def test_state_dict_round_trip_and_torch_accepts_it(ea):
    """10 recorded steps, state_dict(), a fresh DeviceAdam that loads it: 10 more steps are bit-identical to the uninterrupted
    run.  torch.optim.Adam loads the same dict (the three extra keys dropped); after the same 10 further steps it is within
    4 x e32 + 1e-7 of the float64 continuation, e32 = the error of the device continuation (float32) against the same."""
    import torch
    from evacuation_amd import trainer
    D = 6
    gen = torch.Generator().manual_seed(12)
    base = make_net(D, seed=2)
    grads = [[g.to(DEV) for g in _random_grads(base, gen, SCALES[k % 4] * 0.05)] for k in range(20)]

    def run(net, opt, ks):
        for k in ks:
            opt.param_groups[0]["lr"] = 3e-4 * (1 - k / 40)
            sq = torch.zeros((), device=DEV)
            with torch.no_grad():
                for p, g in zip(R.mlp_tensors(net), grads[k]):
                    p.grad.copy_(g)
                    sq = sq + (g * g).sum()
            opt.step(sq)

    net_a = twin(2, D, base)
    opt_a = trainer.DeviceAdam(net_a)
    run(net_a, opt_a, range(20))
    net_b = twin(2, D, base)
    opt_b = trainer.DeviceAdam(net_b)
    run(net_b, opt_b, range(10))
    sd = opt_b.state_dict()
    assert int(sd["state"][0]["step"]) == 10 and set(sd["state"]) == set(range(13)) and sd["param_groups"][0]["eps"] == 1e-5
    mid = [p.detach().clone() for p in R.mlp_tensors(net_b)]
    net_c = twin(2, D, net_b)
    opt_c = trainer.DeviceAdam(net_c, lr=1.0, eps=1.0)                        # (overwritten by the dict)
    opt_c.load_state_dict(sd)
    hc, hb = opt_c.read_header(), opt_b.read_header()
    assert (hc["t"], hc["P1"], hc["P2"]) == (hb["t"], hb["P1"], hb["P2"]) and hc["t"] == 10
    run(net_c, opt_c, range(10, 20))
    assert_same_state(snapshot(net_c, opt_c), snapshot(net_a, opt_a), "state dict", grads=True)
    # without the running products: beta ** step
    plain = {"state": sd["state"], "param_groups": [{k: v for k, v in sd["param_groups"][0].items() if k not in ("P1", "P2", "max_grad_norm")}]}
    opt_e = trainer.DeviceAdam(twin(2, D, net_b))
    opt_e.load_state_dict(plain)
    h = opt_e.read_header()
    assert h["t"] == 10 and h["P1"] == 0.9 ** 10 and h["P2"] == 0.999 ** 10

    def torch_continue(dtype):
        P = [p.to(dtype).clone().requires_grad_(True) for p in mid]
        o = torch.optim.Adam(P, lr=3e-4, eps=1e-5)
        o.load_state_dict({"state": {i: {k: v.clone() for k, v in st.items()} for i, st in plain["state"].items()},
                           "param_groups": [dict(plain["param_groups"][0])]})
        assert float(o.state[P[0]]["step"]) == 10 and o.state[P[0]]["exp_avg"].dtype == dtype
        for k in range(10, 20):
            o.param_groups[0]["lr"] = 3e-4 * (1 - k / 40)
            for p, g in zip(P, grads[k]):
                p.grad = g.to(dtype).clone()
            torch.nn.utils.clip_grad_norm_(P, 0.5)
            o.step()
        return [p.detach().double() for p in P]

    p64, p32 = torch_continue(torch.float64), torch_continue(torch.float32)
    pk = [p.detach().double() for p in R.mlp_tensors(net_a)]
    e32 = max(float((x - y).abs().max()) for x, y in zip(pk, p64))
    et = max(float((x - y).abs().max()) for x, y in zip(p32, p64))
    moved = max(float((x - y.double()).abs().max()) for x, y in zip(p64, mid))
    print(f"\nstate dict: device continuation vs float64 e32 = {e32:.3e}; torch float32 loaded from the dict vs float64 = {et:.3e}; moved {moved:.3e}")
    assert moved > 1e-4
    assert et <= 4 * e32 + 1e-7, (et, e32)


# ------------------------------------------------------------------------------------------------ RPOTrainer(optimizer="device")
def _two_updates(ea, **kw):
    import torch
    tr = make_trainer(ea, 10, 64, 64, total_timesteps=64 * 64 * 2, num_minibatches=4, update_epochs=3, optimizer="device", **kw)
    logs = tr.learn()
    torch.cuda.synchronize()
    assert len(logs) == 2 and all(math.isfinite(l["loss"]) and math.isfinite(l["clipfrac"]) for l in logs)
    out = SimpleNamespace(params=[p.detach().clone() for p in R.mlp_tensors(tr.net)], logs=logs, steps=tr.minibatch_steps,
                          t=tr.optimizer.step_count)
    tr.env.close()
    return out


def test_device_trainer_is_bit_reproducible_and_one_call_equals_per_minibatch_calls(ea):
    runs = {}
    for name, kw in (("one", {}), ("again", {}), ("per", {"one_call": False}), ("one_kl", {"target_kl": 0.004}),
                     ("per_kl", {"one_call": False, "target_kl": 0.004})):
        runs[name] = _two_updates(ea, **kw)
    for x, y in (("one", "again"), ("one", "per"), ("one_kl", "per_kl")):
        for a, b in zip(runs[x].params, runs[y].params):
            assert same_bits(a, b), (x, y)
        assert runs[x].steps == runs[y].steps == runs[x].t == runs[y].t
        for la, lb in zip(runs[x].logs, runs[y].logs):
            assert set(la) == set(lb)
            for k in ("loss", "value_loss", "policy_loss", "entropy", "old_approx_kl", "approx_kl", "learning_rate"):
                assert la[k] == lb[k], (x, y, k)
            assert abs(la["clipfrac"] - lb["clipfrac"]) <= 1e-6
    assert runs["one"].steps == 2 * 3 * 4
    print("\nsteps with target_kl = 0.004:", runs["one_kl"].steps, "of", runs["one"].steps)


def test_device_loop_wiring_against_the_yardstick_driven_loops(ea):
    """The wiring test of tests/test_gpu_trainer.py for the device forms: one short update (1 epoch x 4 minibatches, 64 envs x 32
    steps, injected RPO noise) from one seed on twin envs: kernels + device optimiser (one call, and per-minibatch calls),
    yardstick float32 and float64 with torch's optimiser.  Collection, advantages, permutations and noise are identical bit for
    bit; the device-driven parameters lie within 4 x d32 + 1e-7 of the float64-driven ones, d32 measured from the float32-driven."""
    import torch
    runs = {}
    for name, dtype, kw in (("one", None, {"optimizer": "device"}), ("per", None, {"optimizer": "device", "one_call": False}),
                            ("f32", torch.float32, {}), ("f64", torch.float64, {})):
        gen = torch.Generator(device=DEV).manual_seed(99)
        alpha = 0.5
        noises = []

        def noise_fn(M, gen=gen, noises=noises):
            z = (torch.rand(M, 2, device=DEV, generator=gen) * 2 - 1) * alpha
            noises.append(z)
            return z
        hooks = dict(kw, rpo_noise_fn=noise_fn)
        if dtype is not None:
            hooks["grad_fn"] = _yardstick_grad_fn(dtype, {})
        tr = make_trainer(ea, 10, 64, 32, total_timesteps=64 * 32, num_minibatches=4, update_epochs=1, rpo_alpha=alpha, **hooks)
        tr.update()
        torch.cuda.synchronize()
        runs[name] = SimpleNamespace(params=[p.detach().double().clone() for p in R.mlp_tensors(tr.net)],
                                     storage={k: v.clone() for k, v in tr.storage.items()}, adv=tr.advantages.clone(),
                                     perms=[p.clone() for p in tr.last_permutations], noises=[z.clone() for z in noises])
        tr.env.close()
    a, b = runs["f32"], runs["f64"]
    d32 = max(float((x - y).abs().max()) for x, y in zip(a.params, b.params))
    moved = max(float((x - y.double()).abs().max()) for x, y in zip(b.params, [p.detach() for p in R.mlp_tensors(make_initial_net(6))]))
    assert moved > 1e-4
    for name in ("one", "per"):
        k = runs[name]
        for other in (a, b):
            for key in k.storage:
                assert torch.equal(k.storage[key].view(torch.int32), other.storage[key].view(torch.int32)), key
            assert torch.equal(k.adv, other.adv)
            assert len(k.perms) == 1 and torch.equal(k.perms[0], other.perms[0])
            assert len(k.noises) == 4 and all(torch.equal(x, y) for x, y in zip(k.noises, other.noises))
        dk = max(float((x - y).abs().max()) for x, y in zip(k.params, b.params))
        print(f"\ndevice loop wiring ({name}): d32 = {d32:.3e}, device-driven vs float64-driven = {dk:.3e}, bound {4 * d32 + 1e-7:.3e}; moved {moved:.3e}")
        assert dk <= 4 * d32 + 1e-7, (name, dk, d32)
    for x, y in zip(runs["one"].params, runs["per"].params):
        assert torch.equal(x, y)


def test_custom_grad_fn_with_the_device_optimiser(ea):
    import torch
    tr = make_trainer(ea, 10, 64, 32, total_timesteps=64 * 32, num_minibatches=4, update_epochs=2, optimizer="device",
                      grad_fn=_yardstick_grad_fn(torch.float32, {}), rpo_noise_fn=lambda M: torch.zeros(M, 2, device=DEV))
    before = [p.detach().clone() for p in R.mlp_tensors(tr.net)]
    log = tr.update()
    torch.cuda.synchronize()
    assert math.isfinite(log["loss"]) and tr.optimizer.step_count == 8 and tr.minibatch_steps == 8
    assert all(bool(torch.isfinite(p).all()) for p in R.mlp_tensors(tr.net))
    assert max(float((p.detach() - q).abs().max()) for p, q in zip(R.mlp_tensors(tr.net), before)) > 1e-4
    tr.env.close()


def test_the_device_loop_learns(ea):
    """The learning smoke test of tests/test_gpu_trainer.py with optimizer="device", its set-up taken over unchanged (N = 10,
    256 envs x 128 steps, 4 minibatches x 4 epochs, 40 updates, episodes cut at 100 steps): the mean episodic return of the last
    5 updates exceeds that of the first 5."""
    tr = make_trainer(ea, 10, 256, 128, total_timesteps=256 * 128 * 40, num_minibatches=4, update_epochs=4, max_timesteps=100,
                      optimizer="device")
    means = []
    for log in tr.learn():
        r = log["episodes"]["episode_reward"]
        assert r.numel() >= 256
        means.append(float(r.mean()))
    tr.env.close()
    print("\nlearning (device optimiser, one call per update): mean episodic return per update:", " ".join(f"{m:.1f}" for m in means))
    assert len(means) == 40
    first, last = sum(means[:5]) / 5, sum(means[-5:]) / 5
    assert last > first, (first, last)
