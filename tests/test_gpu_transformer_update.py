"""GPU tests of the transformer leader's optimiser step and whole update: evac_transformer_adam_step bit for bit against the
NumPy statement of its arithmetic over all 13 + 16 per block tensors (tests/optimizer_ref.py) with canaries behind every tensor
and around a block that is not in use, a NaN sum of squares, evac_transformer_minibatch_step == gradient call + step call, graph
capture (the step count lives on the device), evac_transformer_update == the host loop of minibatch steps including the early
exit at target_kl taken on the device, determinism on two streams, RPOTrainer(grad_fn=transformer_kernel_grad,
optimizer="device_transformer") with a state_dict round trip, and the example.

Shapes (N, dm, blocks, use_resid), the smallest at which the walk over the tensors can go wrong:
  (1, 2, 1, False)    D = 6, 29 tensors, every encoder tensor smaller than a workgroup
  (10, 3, 2, False)   D = 36, 45 tensors
  (62, 6, 2, True)    D = 384, 64 tokens; ff1_w = 576 elements = 2 1/4 workgroups; actor_w1 = 96 workgroups
Bit for bit means: the float32 / int64 / float64 words are compared as integers.  No tolerance anywhere: the kernel's arithmetic
is adam_element's, whose sequence AdamRef restates."""
import ctypes as C
import math
import os
import re
import subprocess
import sys
from types import SimpleNamespace

import numpy as np
import pytest

from tests import transformer_grad_cases as TC
from tests.optimizer_ref import AdamRef
from tests.trainer_cases import DEV, loss_cfg, same_bits
from tests.workspace_guard import CANARY, Guarded

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHAPES = [(1, 2, 1, False), (10, 3, 2, False), (62, 6, 2, True)]


@pytest.fixture(scope="module")
def ea():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("needs an MI355X")
    import evacuation_amd
    return evacuation_amd


def make_twins(shape, seed, n=2):
    """``n`` networks of tests/transformer_grad_cases.make_net with the same parameters (the same seed) and nothing shared."""
    nets = [TC.make_net(*shape, seed=seed) for _ in range(n)]
    for other in nets[1:]:
        assert all(same_bits(p, q) for p, q in zip(TC.all_tensors(nets[0]), TC.all_tensors(other)))
    return nets


def make_batch(net, B, seed):
    """A batch of B rows for ``net``: old log-probabilities and values near the network's own, so ratios on both sides of 1."""
    import torch
    g = torch.Generator().manual_seed(seed)
    D = int(TC.all_tensors(net)[0].shape[1])
    obs = (0.6 * torch.randn(B, D, generator=g)).clamp(-1, 1).to(DEV)
    act = torch.randn(B, 2, generator=g).to(DEV)
    with torch.no_grad():
        _, lp, _, val = net.get_action_and_value(obs, act)
    batch = {"b_obs": obs, "b_actions": act, "b_logprobs": lp + 0.2 * torch.randn(B, generator=g).to(DEV),
             "b_advantages": (torch.randn(B, generator=g) + 0.3).to(DEV), "b_returns": val.view(-1) + 0.7 * torch.randn(B, generator=g).to(DEV),
             "b_values": val.view(-1) + 0.1 * torch.randn(B, generator=g).to(DEV)}
    return {k: v.float().contiguous() for k, v in batch.items()}


def snapshot(net, opt):
    import torch
    torch.cuda.synchronize()
    ts = TC.all_tensors(net)
    assert len(ts) == len(opt.exp_avg) == len(opt.exp_avg_sq) == len(opt.params)
    return SimpleNamespace(params=[p.detach().clone() for p in ts], grads=[p.grad.detach().clone() for p in ts],
                           m=[t.clone() for t in opt.exp_avg], v=[t.clone() for t in opt.exp_avg_sq], header=opt.read_header())


def assert_same_state(a, b, what):
    names = TC.names((len(a.params) - 13) // 16)
    for name in ("params", "m", "v", "grads"):
        for i, (x, y) in enumerate(zip(getattr(a, name), getattr(b, name))):
            assert same_bits(x, y), (what, name, names[i], float((x - y).abs().max()))
    for k in ("t", "P1", "P2"):
        assert a.header[k] == b.header[k], (what, k, a.header, b.header)


# ------------------------------------------------------------------------------------------------ evac_transformer_adam_step
@pytest.mark.parametrize("N,dm,blocks,resid", SHAPES)
def test_adam_step_is_bit_equal_to_the_yardstick(ea, N, dm, blocks, resid):
    """Three consecutive steps of the C entry on random parameters and gradients, the sum of squares above the clip threshold,
    below it, above it: all tensors x {parameter, clipped gradient, exp_avg, exp_avg_sq} and (t, P1, P2) after every step; the
    canaries behind every tensor, and with one block those that blocks[1] points at, are as they were."""
    import torch
    from evacuation_amd import _lib
    from evacuation_amd.policy import _transformer_grads
    from evacuation_amd.trainer import decode_header
    lib = _lib.load()
    net = TC.make_net(N, dm, blocks, resid, seed=N, device="cpu")
    shapes = [tuple(p.shape) for p in TC.all_tensors(net)]
    nt = 13 + 16 * blocks
    assert len(shapes) == nt and shapes[0] == (64, (N + 2) * dm)
    assert sum(int(np.prod(s)) for s in shapes[13:29]) == 4 * 3 * dm * dm + 3 * 3 * dm + 2 * 96 * dm + 96 + 6 * dm
    rng = np.random.default_rng(100 + N)
    ref_params = [rng.uniform(-0.5, 0.5, s).astype(np.float32) for s in shapes]
    zeros = [np.zeros(s, np.float32) for s in shapes]
    sets = {k: Guarded(a) for k, a in (("p", ref_params), ("g", zeros), ("m", zeros), ("v", zeros))}
    unused = Guarded([np.full(600, CANARY, np.float32) for _ in range(4 * 16)])  # what a block not in use points at
    header = torch.zeros(8, dtype=torch.int64, device=DEV)
    sumsq_dev = torch.zeros(1, dtype=torch.float32, device=DEV)

    def structs(k, which):
        ptrs = sets[k].ptrs()
        enc = _transformer_grads(*ptrs[13:])
        if blocks == 1:
            enc.blocks[1] = _lib.EvacTransformerBlockGrads(*unused.ptrs()[16 * which:16 * which + 16])
        return _lib.EvacMlpPolicyGrads(*ptrs[:13]), enc
    (p13, penc), (g13, genc), (m13, menc), (v13, venc) = (structs(k, i) for i, k in enumerate("pgmv"))
    state = _lib.EvacTransformerAdamState(header.data_ptr(), m13, v13, menc, venc)
    ref = AdamRef(ref_params, np.float32, lr=3e-4, eps=1e-5, max_grad_norm=0.5)
    coefs = []
    for k, scale in enumerate((10.0, 1e-4, 1.0)):
        lr = 3e-4 * (1.0 - k / 3)
        g_np = [(scale * rng.standard_normal(s)).astype(np.float32) for s in shapes]
        sumsq = np.float32(0)
        for g in g_np:
            sumsq = np.float32(sumsq + np.sum(np.square(g, dtype=np.float32), dtype=np.float32))
        for v, g in zip(sets["g"].views, g_np):
            v.copy_(torch.from_numpy(g.reshape(-1)))
        sumsq_dev.fill_(float(sumsq))
        cfg = _lib.EvacAdamConfig(lr, 0.9, 0.999, 1e-5, 0.5)
        rc = lib.evac_transformer_adam_step(C.byref(p13), C.byref(penc), C.byref(g13), C.byref(genc), C.byref(state), C.byref(cfg),
                                            (N + 2) * dm, dm, blocks, sumsq_dev.data_ptr(), torch.cuda.current_stream().cuda_stream)
        assert rc == 0, rc
        torch.cuda.synchronize()
        ref.lr = lr
        ref.step(ref_params, g_np, sumsq)
        coefs.append(float(ref.last_clip_coef))
        for name, key, want in (("param", "p", ref_params), ("grad", "g", g_np), ("exp_avg", "m", ref.exp_avg), ("exp_avg_sq", "v", ref.exp_avg_sq)):
            for i, (got, host) in enumerate(zip(sets[key].host(shapes), want)):
                assert np.array_equal(got.view(np.int32), host.view(np.int32)), \
                    ((N, dm, blocks, k), name, TC.names(blocks)[i], int((got.view(np.int32) != host.view(np.int32)).sum()))
        h = decode_header(header)
        assert (h["t"], h["P1"], h["P2"]) == (ref.t, ref.P1, ref.P2), (k, h, ref.t, ref.P1, ref.P2)
        for key, s in sets.items():
            assert s.canaries_intact(), (k, key)
        assert unused.canaries_intact() and bool((unused.buf == CANARY).all()), k
    assert coefs[0] < 1.0 and coefs[1] == 1.0 and coefs[2] < 1.0, coefs        # both branches of the clip
    assert decode_header(header)["t"] == 3


def test_a_nan_sum_of_squares_makes_everything_nan_and_counts(ea):
    import torch
    from evacuation_amd.trainer import TransformerAdam
    net = TC.make_net(10, 3, 2, False, seed=1)
    opt = TransformerAdam(net)
    assert len(opt.params) == 45 and opt.num_blocks == 2 and opt.elem_dim == 3
    with torch.no_grad():
        for p in TC.all_tensors(net):
            p.grad.normal_()
    opt.step(torch.tensor([float("nan")], dtype=torch.float32, device=DEV))
    torch.cuda.synchronize()
    for name, p, m, v in zip(TC.names(2), TC.all_tensors(net), opt.exp_avg, opt.exp_avg_sq):
        assert bool(torch.isnan(p).all()) and bool(torch.isnan(m).all()) and bool(torch.isnan(v).all()), name
    assert opt.read_header()["t"] == 1 and opt.step_count == 1


# ------------------------------------------------------------------------------------------------ evac_transformer_minibatch_step
@pytest.mark.parametrize("shape,M", list(zip(SHAPES, (2, 64, 300))))
@pytest.mark.parametrize("norm_adv", [1, 0])
def test_minibatch_step_equals_gradient_then_adam(ea, shape, M, norm_adv):
    """Two consecutive steps (the second from non-zero moments) with injected noise: one call against gradient call + step call
    on a twin network, bit for bit: parameters, moments, clipped gradients, statistics, header."""
    import torch
    from evacuation_amd import trainer
    cfg = loss_cfg(norm_adv, 1, 0.01, 0.5)
    net_a, net_b = make_twins(shape, seed=7 + M)
    B = 2 * M + 3
    batch = make_batch(net_a, B, seed=M)
    g = torch.Generator().manual_seed(M + norm_adv)
    inds = torch.randint(0, B, (M,), generator=g).to(DEV)
    z = ((torch.rand(M, 2, generator=g) * 2 - 1) * cfg.rpo_alpha).to(DEV).contiguous()
    opt_a, opt_b = trainer.TransformerAdam(net_a, lr=1e-3), trainer.TransformerAdam(net_b, lr=1e-3)
    assert len(opt_a.params) == 13 + 16 * shape[2]
    if shape[2] == 1:                                                         # a block not in use is NULL everywhere, and accepted
        for st in (opt_b.encoder_params_struct(), trainer.ensure_encoder_grads(net_b), opt_b.state_struct().enc_exp_avg,
                   opt_b.state_struct().enc_exp_avg_sq):
            assert all(getattr(st.blocks[1], f) is None for f in TC.BLOCK_NAMES) and st.blocks[0].wq
    clipped = 0
    for k in range(2):
        stats_a = trainer.transformer_minibatch_grad(net_a, batch, inds, cfg, rpo_noise=z)
        unclipped = [p.grad.detach().clone() for p in TC.all_tensors(net_a)]
        opt_a.step(stats_a[7])
        stats_b = trainer.transformer_minibatch_step(net_b, batch, inds, cfg, opt_b, rpo_noise=z)
        a, b = snapshot(net_a, opt_a), snapshot(net_b, opt_b)
        assert_same_state(a, b, (shape, M, norm_adv, k))
        assert same_bits(stats_a, stats_b), (stats_a, stats_b)
        assert a.header == b.header and a.header["t"] == k + 1 and a.header["stop"] == 0
        assert all(bool(torch.isfinite(p).all()) for p in b.params)
        if min(1.0, 0.5 / (math.sqrt(float(stats_a[7])) + 1e-6)) < 0.99:          # .grad holds the CLIPPED gradient, stats[7] the unclipped sum
            clipped += 1
            assert any(not same_bits(u, gr) for u, gr in zip(unclipped, b.grads))
    print(f"\n{shape} M = {M}: {clipped} of 2 steps clipped")


def test_captured_step_counts_when_replayed(ea):
    """One transformer_minibatch_step captured; the minibatch indices and the injected noise rewritten in place between replays:
    3 replays == 3 direct calls from the same start; the header counts 3."""
    import torch
    from evacuation_amd import trainer
    cfg = loss_cfg(1, 1, 0.01, 0.5)
    shape, M, B = SHAPES[1], 64, 131
    net, direct_net = make_twins(shape, seed=21)
    batch = make_batch(net, B, seed=21)
    start = [p.detach().clone() for p in TC.all_tensors(net)]
    gen = torch.Generator().manual_seed(3)
    all_inds = [torch.randint(0, B, (M,), generator=gen).to(DEV) for _ in range(4)]
    all_z = [((torch.rand(M, 2, generator=gen) * 2 - 1) * cfg.rpo_alpha).to(DEV) for _ in range(4)]
    inds, z, stats = all_inds[3].clone(), all_z[3].clone(), torch.zeros(8, device=DEV)
    opt = trainer.TransformerAdam(net, lr=1e-3)
    trainer.transformer_minibatch_step(net, batch, inds, cfg, opt, rpo_noise=z, stats=stats)   # warm-up: binds, allocates ...
    torch.cuda.synchronize()
    with torch.no_grad():                                                                    # ... and is undone, in place
        for p, s in zip(TC.all_tensors(net), start):
            p.copy_(s)
        for t in opt.exp_avg + opt.exp_avg_sq:
            t.zero_()
        opt.header.zero_()
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        trainer.transformer_minibatch_step(net, batch, inds, cfg, opt, rpo_noise=z, stats=stats)
    replayed_stats = []
    for i in range(3):
        inds.copy_(all_inds[i])
        z.copy_(all_z[i])
        graph.replay()
        replayed_stats.append(stats.clone())
    torch.cuda.synchronize()
    direct_opt = trainer.TransformerAdam(direct_net, lr=1e-3)
    for i in range(3):
        s = trainer.transformer_minibatch_step(direct_net, batch, all_inds[i], cfg, direct_opt, rpo_noise=all_z[i])
        assert same_bits(s, replayed_stats[i]), i
    a, b = snapshot(net, opt), snapshot(direct_net, direct_opt)
    assert_same_state(a, b, "graph")
    assert a.header["t"] == 3 and a.header["steps_run"] == 3
    assert not same_bits(a.params[0], start[0]) and not same_bits(a.params[13], start[13]) and not same_bits(a.params[44], start[44])


# ------------------------------------------------------------------------------------------------ evac_transformer_update
def host_loop(trainer, net, batch, perms, cfg, opt, M, noise, seed, first, stats, target_kl=None):
    """The Python loop of minibatch steps that evac_transformer_update replaces, with the host-side early exit; (steps, epochs)."""
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
            last = trainer.transformer_minibatch_step(net, batch, inds, cfg, opt, rpo_noise=None if noise is None else noise[k, :m],
                                                      seed=seed, draw_counter=first + k, stats=stats[k])
            k += 1
        epochs += 1
        if target_kl is not None and float(last[5]) > target_kl:
            break
    return k, epochs


UPDATE_CASES = [  # shape, B, M, norm_adv, epochs, injected noise, steps per epoch
    (SHAPES[0], 70, 32, 0, 3, False, 3),         # one block; a tail of 6 that runs
    (SHAPES[1], 200, 64, 1, 2, False, 4),        # a tail of 8 that runs, drawn noise
    (SHAPES[1], 193, 64, 1, 2, True, 3),         # B mod M == 1 with norm_adv: the tail is skipped; injected noise
    (SHAPES[2], 136, 64, 1, 2, True, 3)]         # 64 tokens, a tail of 8


@pytest.mark.parametrize("shape,B,M,norm_adv,n_epochs,inject,per_epoch", UPDATE_CASES)
def test_update_equals_the_host_loop(ea, shape, B, M, norm_adv, n_epochs, inject, per_epoch):
    import torch
    from evacuation_amd import trainer
    cfg = loss_cfg(norm_adv, 1, 0.01, 0.5)
    net_a, net_b = make_twins(shape, seed=40 + B)
    batch = make_batch(net_a, B, seed=B)
    assert len(trainer.update_steps(B, M, bool(norm_adv))) == per_epoch
    steps = n_epochs * per_epoch
    gen = torch.Generator().manual_seed(B)
    perms = torch.stack([torch.randperm(B, generator=gen) for _ in range(n_epochs)]).to(DEV)
    noise = ((torch.rand(steps, M, 2, generator=gen) * 2 - 1) * cfg.rpo_alpha).to(DEV).contiguous() if inject else None
    opt_a, opt_b = trainer.TransformerAdam(net_a, lr=1e-3), trainer.TransformerAdam(net_b, lr=1e-3)
    stats_a = torch.full((steps, 8), -7.0, device=DEV)
    stats_b = torch.full((steps, 8), -7.0, device=DEV)
    out, header = trainer.transformer_update(net_a, batch, perms, cfg, opt_a, rpo_noise=noise, seed=11, first_draw_counter=1000,
                                             stats=stats_a, minibatch_size=M)
    assert out is stats_a
    ran, epochs = host_loop(trainer, net_b, batch, perms, cfg, opt_b, M, noise, 11, 1000, stats_b)
    a, b = snapshot(net_a, opt_a), snapshot(net_b, opt_b)
    assert (ran, epochs) == (steps, n_epochs)
    h = trainer.decode_header(header)
    assert (h["steps_run"], h["epochs_run"], h["stop"], h["t"]) == (steps, n_epochs, 0, steps), h
    assert_same_state(a, b, (shape, B, M))
    assert same_bits(stats_a, stats_b)
    assert not bool((stats_a == -7.0).any())
    assert all(bool(torch.isfinite(p).all()) for p in a.params)


def test_target_kl_is_taken_on_the_device(ea):
    """target_kl = 0.0, 3 epochs of 4 minibatches: approx_kl = mean((r - 1) - log r) is >= 0 and > 0 once an earlier step of the
    epoch has moved the parameters, so the call stops after the first epoch, as the host loop with its break does; the rows of
    stats beyond steps_run keep the sentinel.  With target_kl = 1e9 nothing stops."""
    import torch
    from evacuation_amd import trainer
    shape, B, M, n_epochs = SHAPES[1], 256, 64, 3
    cfg = loss_cfg(1, 1, 0.01, 0.5)
    net0 = TC.make_net(*shape, seed=77)
    batch = make_batch(net0, B, seed=77)
    gen = torch.Generator().manual_seed(8)
    perms = torch.stack([torch.randperm(B, generator=gen) for _ in range(n_epochs)]).to(DEV)
    per_epoch, steps = B // M, n_epochs * (B // M)

    def fresh():
        net = TC.make_net(*shape, seed=77)
        return net, trainer.TransformerAdam(net, lr=1e-3)
    cfg.target_kl = 0.0
    try:
        net_h, opt_h = fresh()
        stats_h = torch.full((steps, 8), -7.0, device=DEV)
        ran_h, epochs_h = host_loop(trainer, net_h, batch, perms, cfg, opt_h, M, None, 5, 0, stats_h, target_kl=cfg.target_kl)
        assert (ran_h, epochs_h) == (per_epoch, 1) and float(stats_h[per_epoch - 1, 5]) > 0.0, stats_h[:, 5]
        net_d, opt_d = fresh()
        stats_d = torch.full((steps, 8), -7.0, device=DEV)
        _, header = trainer.transformer_update(net_d, batch, perms, cfg, opt_d, seed=5, first_draw_counter=0, stats=stats_d, minibatch_size=M)
        a, b = snapshot(net_d, opt_d), snapshot(net_h, opt_h)
        h = trainer.decode_header(header)
        assert (h["epochs_run"], h["steps_run"], h["stop"], h["t"]) == (1, per_epoch, 1, per_epoch), h
        assert_same_state(a, b, "target_kl")
        assert same_bits(stats_d, stats_h)
        assert bool((stats_d[per_epoch:] == -7.0).all()) and not bool((stats_d[:per_epoch] == -7.0).any())
        # a target nothing reaches: a later call clears the flag and runs every epoch
        cfg.target_kl = 1e9
        _, header = trainer.transformer_update(net_d, batch, perms, cfg, opt_d, seed=5, stats=stats_d, minibatch_size=M)
        h = trainer.decode_header(header)
        assert (h["stop"], h["steps_run"], h["epochs_run"], h["t"]) == (0, steps, n_epochs, per_epoch + steps), h
        assert not bool((stats_d == -7.0).any())
    finally:
        cfg.target_kl = None


def test_the_same_update_twice_gives_the_same_bits(ea):
    """Determinism of the whole step: transformer_update (drawn perturbations) from the same start on twin networks, once on the
    current stream and once on a side stream."""
    import torch
    from evacuation_amd import trainer
    shape, B, M = SHAPES[1], 200, 64
    cfg = loss_cfg(1, 1, 0.01, 0.5)
    nets = make_twins(shape, seed=40 + B)
    batch = make_batch(nets[0], B, seed=B)
    gen = torch.Generator().manual_seed(2)
    perms = torch.stack([torch.randperm(B, generator=gen) for _ in range(2)]).to(DEV)
    side = torch.cuda.Stream()
    out = []
    for i, net in enumerate(nets):
        opt = trainer.TransformerAdam(net, lr=1e-3)
        torch.cuda.synchronize()
        if i == 0:
            stats, _ = trainer.transformer_update(net, batch, perms, cfg, opt, seed=9, first_draw_counter=3, minibatch_size=M)
        else:
            with torch.cuda.stream(side):
                stats, _ = trainer.transformer_update(net, batch, perms, cfg, opt, seed=9, first_draw_counter=3, minibatch_size=M)
            side.synchronize()
        out.append((snapshot(net, opt), stats.clone()))
    assert_same_state(out[0][0], out[1][0], "twice")
    assert out[0][0].header == out[1][0].header and out[0][0].header["t"] == 8
    assert same_bits(out[0][1], out[1][1])


# ------------------------------------------------------------------------------------------------ RPOTrainer
LOGGED = ("loss", "value_loss", "policy_loss", "entropy", "old_approx_kl", "approx_kl", "learning_rate")


def _make_trainer(ea, target_kl=None, **hooks):
    import torch
    from evacuation_amd import trainer
    from evacuation_amd.policy import TransformerActorCritic
    cfg = trainer.RPOTrainingConfig(seed=3, num_envs=8, num_steps=16, total_timesteps=8 * 16 * 2, num_minibatches=2, update_epochs=2,
                                    target_kl=target_kl)
    assert cfg.anneal_lr
    env = ea.NormalizedVectorEnv.make(ea.EnvConfig(number_of_pedestrians=10), ea.EnvWrappersConfig(positions="rel", statuses="ohe", type="Box"),
                                      num_envs=8, gamma=cfg.gamma, seed=3)
    torch.manual_seed(0)
    net = TransformerActorCritic(env.obs_dim, 10).to(DEV)
    return trainer.RPOTrainer(env, net, cfg, **hooks)


@pytest.mark.parametrize("target_kl", [None, 0.0])
def test_trainer_with_the_device_optimiser(ea, target_kl):
    """N = 10, the rel + ohe Box observation, 8 envs x 16 steps, 2 minibatches x 2 epochs, two update()s with the learning rate
    annealed: one transformer_update per update and one transformer_minibatch_step per minibatch on twin handles are bit-equal
    after each update, also when target_kl = 0.0 stops every update after its first epoch."""
    import torch
    from evacuation_amd import trainer
    kw = dict(grad_fn=trainer.transformer_kernel_grad, optimizer="device_transformer", target_kl=target_kl)
    one, per = _make_trainer(ea, one_call=True, **kw), _make_trainer(ea, one_call=False, **kw)
    assert isinstance(one.optimizer, trainer.TransformerAdam) and len(one.optimizer.params) == 45
    initial = [p.detach().clone() for p in TC.all_tensors(one.net)]
    per_update = 2 * (1 if target_kl is not None else 2)
    for u in range(2):
        la, lb = one.update(), per.update()
        a, b = snapshot(one.net, one.optimizer), snapshot(per.net, per.optimizer)
        assert_same_state(a, b, ("trainer", u))
        assert set(la) == set(lb)
        for k in LOGGED:
            assert la[k] == lb[k] and math.isfinite(la[k]), (u, k, la[k], lb[k])
        assert abs(la["clipfrac"] - lb["clipfrac"]) <= 1e-6
        assert one.minibatch_steps == per.minibatch_steps == (u + 1) * per_update
        assert one.optimizer.read_header()["stop"] == int(target_kl is not None)
    assert la["learning_rate"] == 0.5 * 3e-4                                          # anneal_lr: the second of two updates
    assert one.optimizer.step_count == per.optimizer.step_count == 2 * per_update
    still = [name for name, p, q in zip(TC.names(2), TC.all_tensors(one.net), initial) if torch.equal(p.detach(), q)]
    assert set(still) <= {TC.names(2)[i] for i in TC.key_biases(2)}, still            # (their exact gradient is zero)
    assert all(bool(torch.isfinite(p).all()) for p in TC.all_tensors(one.net))
    # state_dict() -> load_state_dict() into a fresh optimiser of a network with the same parameters continues bit-identically
    other = _make_trainer(ea, one_call=True, **kw)
    with torch.no_grad():
        for p, q in zip(TC.all_tensors(other.net), TC.all_tensors(one.net)):
            p.copy_(q)
    fresh = trainer.TransformerAdam(other.net, lr=1.0)
    sd = one.optimizer.state_dict()
    assert len(sd["state"]) == 45 and sd["param_groups"][0]["params"] == list(range(45))
    fresh.load_state_dict(sd)
    assert fresh.read_header()["t"] == one.optimizer.step_count and fresh.param_groups[0]["lr"] == one.optimizer.param_groups[0]["lr"]
    batch = make_batch(one.net, 40, seed=1)
    inds = torch.arange(32, device=DEV)
    cfg = loss_cfg(1, 1, 0.0, 0.5)
    sa = trainer.transformer_minibatch_step(one.net, batch, inds, cfg, one.optimizer, seed=1, draw_counter=5)
    sb = trainer.transformer_minibatch_step(other.net, batch, inds, cfg, fresh, seed=1, draw_counter=5)
    assert same_bits(sa, sb)
    assert_same_state(snapshot(one.net, one.optimizer), snapshot(other.net, fresh), "state_dict")
    for t in (one, per, other):
        t.env.close()


def test_any_other_grad_fn_is_followed_by_the_optimisers_own_step(ea):
    import torch
    from evacuation_amd import trainer
    auto = _make_trainer(ea, grad_fn=trainer.autograd_minibatch_grad, optimizer="device_transformer")
    before = [p.detach().clone() for p in TC.all_tensors(auto.net)]
    log = auto.update()
    torch.cuda.synchronize()
    assert math.isfinite(log["loss"]) and auto.optimizer.step_count == 4 and auto.minibatch_steps == 4
    moved = [not torch.equal(p.detach(), q) for p, q in zip(TC.all_tensors(auto.net), before)]
    assert sum(moved) >= 43 and all(bool(torch.isfinite(p).all()) for p in TC.all_tensors(auto.net))
    with pytest.raises(ValueError, match="`embedding`"):
        trainer.RPOTrainer(auto.env, auto.net, auto.cfg, optimizer="device", grad_fn=trainer.transformer_kernel_grad)
    auto.env.close()


def test_train_rpo_example_with_the_device_optimiser(ea):
    cmd = [sys.executable, os.path.join(ROOT, "examples", "train_rpo.py"), "--network", "transformer", "--gradient", "device", "--optimizer",
           "device", "--envs", "8", "--steps", "16", "--updates", "2", "--pedestrians", "10", "--minibatches", "2", "--epochs", "2"]
    done = subprocess.run(cmd, cwd=ROOT, capture_output=True, text=True, timeout=120)
    assert done.returncode == 0, done.stdout[-2000:] + done.stderr[-2000:]
    assert done.stdout.count("SPS:") == 2, done.stdout[-2000:]
    losses = re.findall(r"value_loss=(\S+)\s+policy_loss=(\S+)\s+approx_kl=(\S+)", done.stdout)
    assert len(losses) == 2 and all(math.isfinite(float(x)) for row in losses for x in row), done.stdout[-2000:]
