"""GPU tests of the trainer's update: evac_gae bit for bit against the float32 yardstick, evac_rpo_minibatch_grad against the
float64 yardstick with a tolerance MEASURED per case from torch's own float32 error (tests/trainer_ref.py), determinism, the
device-drawn RPO perturbation, the in-place contract under graph capture, and RPOTrainer's loop (bit-reproducible, wired as the
yardstick-driven loop, and learning).

Tolerance of the gradient cases (nothing fixed in advance): per tensor err = max|g - g64| / max|g64|; e32(case) = the largest
error of the 13 tensors of the float32 yardstick run by torch on the GPU; the kernel must stay within 4 x e32(case) + 1e-7 for
every tensor.  The factor 4 is room for a different but fixed summation order over up to 16 384 samples.  The statistics the same
way, their error taken relative to max(|s64|, 0.1): they are means of per-sample terms of magnitude 0.1 .. 1 (log-ratios, squared
value errors), and a float32 mean's rounding error scales with the terms, not with a mean that cancels to nearly zero
(old_approx_kl); the sum of squares is relative to itself.  The table is printed (run with -s) and copied into DESIGN.md."""
import math
from types import SimpleNamespace

import numpy as np
import pytest

from tests import trainer_ref as R
from tests.trainer_cases import DEV, _yardstick_grad_fn, build_case, loss_cfg, make_initial_net, make_net, make_trainer

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ea():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("needs an MI355X")
    import evacuation_amd
    return evacuation_amd


# ------------------------------------------------------------------------------------------------ evac_gae
def _gae_inputs(T, E, seed):
    import torch
    g = torch.Generator().manual_seed(seed)
    r, v = torch.randn(T, E, generator=g), torch.randn(T, E, generator=g)
    d = (torch.rand(T, E, generator=g) < 0.02).float()
    d[0, 0] = 1.0
    d[T - 1, E - 1] = 1.0
    nv, nd = torch.randn(E, generator=g), (torch.rand(E, generator=g) < 0.02).float()
    nd[E // 2] = 1.0
    return r, v, d, nv, nd


def _split_pair():
    """gamma, lambda for which float32(g) * float32(l) != float32(g * l): a kernel that multiplies two floats fails on it."""
    rng = np.random.default_rng(7)
    for _ in range(1000):
        g, l = rng.uniform(0.8, 1.0, 2)
        if np.float32(g) * np.float32(l) != np.float32(g * l):
            return float(g), float(l)
    raise AssertionError("no such pair found")


@pytest.mark.parametrize("T,E", [(1, 1), (2048, 3), (128, 4096), (37, 1000)])
def test_gae_is_bit_equal_to_the_float32_yardstick(ea, T, E):
    import torch
    from evacuation_amd import trainer
    pairs = [(0.99, 0.95), (1.0, 1.0), (0.9, 0.0), _split_pair()]
    g, l = pairs[3]
    assert np.float32(g) * np.float32(l) != np.float32(g * l)
    r, v, d, nv, nd = _gae_inputs(T, E, seed=T + E)
    assert d[0, 0] == 1 and d[T - 1, E - 1] == 1 and nd[E // 2] == 1
    dev = {k: t.to(DEV) for k, t in (("rewards", r), ("values", v), ("dones", d), ("next_value", nv), ("next_done", nd))}
    for gamma, lam in pairs:
        a_ref, r_ref = R.gae(r, v, d, nv, nd, gamma, lam)                 # torch, float32, on the CPU
        adv, ret = trainer.gae(dev, gamma, lam)
        assert torch.equal(adv.cpu(), a_ref) and torch.equal(ret.cpu(), r_ref), (T, E, gamma, lam, float((adv.cpu() - a_ref).abs().max()))
    out = (torch.full((T, E), 9.0, device=DEV), torch.full((T, E), 9.0, device=DEV))
    adv2, ret2 = trainer.gae(dev, *pairs[0], out=out)
    a_ref, r_ref = R.gae(r, v, d, nv, nd, *pairs[0])
    assert adv2 is out[0] and torch.equal(adv2.cpu(), a_ref) and torch.equal(ret2.cpu(), r_ref)


def test_gae_on_the_storage_of_a_policy_rollout(ea):
    import torch
    from evacuation_amd import trainer
    env = ea.NormalizedVectorEnv.make(ea.EnvConfig(number_of_pedestrians=10, max_timesteps=40), ea.EnvWrappersConfig(positions="grav"),
                                      num_envs=96, seed=3)
    net = make_net(env.obs_dim)
    obs, _ = env.reset()
    st = env.policy_rollout(net, 100, obs.clone(), torch.zeros(96, device=DEV))
    assert float(st["dones"].sum()) > 0                                   # episodes end inside the storage (max_timesteps 40)
    adv, ret = trainer.gae(st, 0.99, 0.95)
    cpu = {k: st[k].cpu() for k in ("rewards", "values", "dones", "next_value", "next_done")}
    a_ref, r_ref = R.gae(cpu["rewards"], cpu["values"], cpu["dones"], cpu["next_value"], cpu["next_done"], 0.99, 0.95)
    assert torch.equal(adv.cpu(), a_ref) and torch.equal(ret.cpu(), r_ref)
    env.close()


# ------------------------------------------------------------------------------------------------ evac_rpo_minibatch_grad
def assert_branch_shares(t, cfg, M):
    """Every branch of max / clamp is taken by a known share of the minibatch (cases of at least 64 samples; a minibatch of two
    cannot hold six branches and checks the sizes' edge instead)."""
    if M < 64:
        return
    c = cfg.clip_coef
    low, high = t.ratio < 1 - c, t.ratio > 1 + c
    pos, neg = t.adv > 0, t.adv < 0
    share = lambda m: float(m.double().mean())
    for name, m in (("ratio below, A > 0", low & pos), ("ratio below, A < 0", low & neg), ("ratio above, A > 0", high & pos),
                    ("ratio above, A < 0", high & neg)):
        assert share(m) >= 0.04, (name, share(m))
    assert 0.3 <= share(~low & ~high) <= 0.7
    assert share(t.pg2 > t.pg1) >= 0.1                                        # the clipped term is the larger one: gradient 0
    assert share(t.dv > c) >= 0.12 and share(t.dv < -c) >= 0.12 and 0.3 <= share(t.dv.abs() <= c) <= 0.7
    if cfg.clip_vloss:
        assert share(t.v_clipped > t.v_unclipped) >= 0.05 and share((t.dv.abs() > c) & (t.v_unclipped > t.v_clipped)) >= 0.05


def tensor_errors(grads, g64):
    out = []
    for g, ref in zip(grads, g64):
        scale = float(ref.abs().max())
        out.append(float((g.double() - ref).abs().max()) / (scale if scale > 0 else 1.0))
    return out


def stat_errors(s, s64):
    out = []
    for i in range(8):
        ref = float(s64[i])
        scale = abs(ref) if i == 7 else max(abs(ref), 0.1)
        out.append(abs(float(s[i]) - ref) / (scale if scale > 0 else 1.0))
    return out


def kernel_grad(net, batch, inds, cfg, z, **kw):
    import torch
    from evacuation_amd import trainer
    from evacuation_amd.policy import mlp_tensors
    stats = trainer.rpo_minibatch_grad(net, batch, inds, cfg, rpo_noise=z, **kw)
    torch.cuda.synchronize()
    return [p.grad.clone() for p in mlp_tensors(net)], stats.clone()


#        D    M      mode       norm_adv clip_vloss ent   alpha
CASES = [(6, 2, "repeat", 1, 1, 0.0, 0.5), (6, 64, "strided", 0, 0, 0.01, 0.0), (6, 64, "repeat", 1, 1, 0.01, 0.5),
         (6, 1000, "repeat", 1, 0, 0.0, 0.5), (6, 16384, "strided", 1, 1, 0.01, 0.5), (6, 16384, "repeat", 0, 0, 0.0, 0.0),
         (6, 16384, "strided", 0, 1, 0.01, 0.5), (6, 16384, "repeat", 1, 0, 0.0, 0.0),
         (124, 2, "strided", 0, 1, 0.01, 0.0), (124, 64, "repeat", 1, 1, 0.0, 0.5), (124, 1000, "strided", 0, 0, 0.01, 0.5),
         (124, 1000, "repeat", 0, 1, 0.0, 0.0), (124, 16384, "repeat", 1, 0, 0.0, 0.0), (124, 16384, "strided", 1, 1, 0.01, 0.5),
         (396, 2, "repeat", 1, 0, 0.01, 0.5), (396, 64, "strided", 0, 0, 0.0, 0.0), (396, 1000, "repeat", 1, 1, 0.01, 0.0),
         (396, 1000, "strided", 0, 0, 0.01, 0.5), (396, 16384, "strided", 0, 1, 0.0, 0.5), (396, 16384, "repeat", 1, 0, 0.01, 0.0)]


def test_the_cases_cover_every_axis():
    for D in (6, 124, 396):
        rows = [c for c in CASES if c[0] == D]
        assert {c[1] for c in rows} == {2, 64, 1000, 16384} and {c[2] for c in rows} == {"repeat", "strided"}
        assert {(c[3], c[4]) for c in rows} == {(0, 0), (0, 1), (1, 0), (1, 1)}
        assert {c[5] for c in rows} == {0.0, 0.01} and {c[6] for c in rows} == {0.0, 0.5}
    assert {(c[3], c[4]) for c in CASES if c[1] == 16384} == {(0, 0), (0, 1), (1, 0), (1, 1)}


@pytest.mark.parametrize("D,M,mode,norm_adv,clip_vloss,ent,alpha", CASES)
def test_minibatch_grad_against_the_float64_yardstick(ea, D, M, mode, norm_adv, clip_vloss, ent, alpha):
    cfg = loss_cfg(norm_adv, clip_vloss, ent, alpha)
    net, batch, inds, z, g64, s64, t = build_case(D, M, mode, cfg, seed=D + M)
    assert_branch_shares(t, cfg, M)
    if mode == "repeat" and M >= 64:
        assert int(inds.unique().numel()) < M                                 # indices do repeat
    g32, s32, _ = R.minibatch_grad(net, batch, inds, cfg, z)                  # torch, float32, on the GPU
    gk, sk = kernel_grad(net, batch, inds, cfg, z)
    e32, ek = tensor_errors(g32, g64), tensor_errors(gk, g64)
    se32, sek = stat_errors(s32, s64), stat_errors(sk, s64)
    bound, sbound = 4 * max(e32) + 1e-7, 4 * max(se32) + 1e-7
    print(f"\ncase D={D} M={M} {mode} norm_adv={norm_adv} clip_vloss={clip_vloss} ent={ent} alpha={alpha}: e32(case) = {max(e32):.2e}, "
          f"bound {bound:.2e}; statistics e32 = {max(se32):.2e}, bound {sbound:.2e}")
    for name, a, b in zip(R.NAMES, e32, ek):
        print(f"  {name:13s} torch f32 {a:.2e}   kernel {b:.2e}")
    for name, a, b in zip(R.STATS, se32, sek):
        print(f"  {name:13s} torch f32 {a:.2e}   kernel {b:.2e}")
    for name, b in zip(R.NAMES, ek):
        assert b <= bound, (name, b, bound)
    for name, b in zip(R.STATS, sek):
        assert b <= sbound, (name, b, sbound)


def test_minibatch_grad_is_deterministic(ea):
    import torch
    cfg = loss_cfg(1, 1, 0.01, 0.5)
    net, batch, inds, z, *_ = build_case(124, 16384, "repeat", cfg, seed=5)
    g1, s1 = kernel_grad(net, batch, inds, cfg, z)
    for p in R.mlp_tensors(net):
        p.grad.fill_(7.0)                                                     # written, not accumulated
    junk = [torch.randn(1 << 20, device=DEV) for _ in range(5)]               # unrelated allocations and work
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        g2, s2 = kernel_grad(net, batch, inds, cfg, z)
    side.synchronize()
    del junk
    for a, b in zip(g1, g2):
        assert torch.equal(a, b)
    assert torch.equal(s1, s2)


def test_device_drawn_rpo_noise(ea):
    import torch
    from oracle.philox import _key, philox4x32_10, usym
    cfg = loss_cfg(1, 1, 0.0, 0.5)
    M, seed, counter = 16384, 0x1234567890ABCDEF, (7 << 32) + 5
    net, batch, inds, _, *_ = build_case(6, M, "strided", cfg, seed=9)

    def draws(ctr):
        w = philox4x32_10(np.arange(M, dtype=np.uint64), ctr & 0xFFFFFFFF, ctr >> 32, 0x52504F5A, *_key(seed))
        return np.stack([np.float32(cfg.rpo_alpha) * usym(w[0]), np.float32(cfg.rpo_alpha) * usym(w[1])], axis=-1).astype(np.float32)

    zs = draws(counter)
    assert zs.min() >= -cfg.rpo_alpha and zs.max() <= cfg.rpo_alpha
    n, a = zs.size, cfg.rpo_alpha
    assert abs(zs.mean()) <= 5 * (a / math.sqrt(3)) / math.sqrt(n)                                    # mean 0, variance a^2 / 3
    assert abs(zs.var() - a * a / 3) <= 5 * math.sqrt(4.0 / 45.0) * a * a / math.sqrt(n)               # var of z^2 = 4 a^4 / 45
    gd, sd = kernel_grad(net, batch, inds, cfg, None, seed=seed, draw_counter=counter)
    gi, si = kernel_grad(net, batch, inds, cfg, torch.from_numpy(zs).to(DEV))
    for x, y in zip(gd, gi):
        assert torch.equal(x, y)
    assert torch.equal(sd, si)
    go, _ = kernel_grad(net, batch, inds, cfg, None, seed=seed, draw_counter=counter + 1)
    assert not torch.equal(go[0], gd[0]) and not np.array_equal(draws(counter + 1), zs)


def test_in_place_contract_under_graph_capture(ea):
    import torch
    from evacuation_amd import trainer
    cfg = loss_cfg(1, 1, 0.01, 0.5)
    net, batch, inds, z, *_ = build_case(6, 1000, "strided", cfg, seed=21)
    stats = torch.zeros(8, device=DEV)
    trainer.rpo_minibatch_grad(net, batch, inds, cfg, rpo_noise=z, stats=stats)                       # warm-up: binds, allocates
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        trainer.rpo_minibatch_grad(net, batch, inds, cfg, rpo_noise=z, stats=stats)
    with torch.no_grad():
        for p in R.mlp_tensors(net):
            p.add_(0.05 * torch.randn_like(p))                                                        # in place: same addresses
    graph.replay()
    torch.cuda.synchronize()
    replayed = [p.grad.clone() for p in R.mlp_tensors(net)]
    replayed_stats = stats.clone()
    direct, direct_stats = kernel_grad(net, batch, inds, cfg, z)
    for a, b in zip(replayed, direct):
        assert torch.equal(a, b)
    assert torch.equal(replayed_stats, direct_stats)
    g64, _, _ = R.minibatch_grad(net, batch, inds, cfg, z, torch.float64)                             # ... and they are the new parameters' gradients
    assert max(tensor_errors(replayed, g64)) < 1e-4


# ------------------------------------------------------------------------------------------------ RPOTrainer
def test_update_is_bit_reproducible(ea):
    import torch
    finals = []
    for _ in range(2):
        tr = make_trainer(ea, 10, 64, 64, total_timesteps=64 * 64 * 2, num_minibatches=4, update_epochs=2)
        logs = tr.learn()
        assert len(logs) == 2 and all(math.isfinite(l["loss"]) for l in logs)
        torch.cuda.synchronize()
        finals.append([p.detach().clone() for p in R.mlp_tensors(tr.net)])
        tr.env.close()
    for a, b in zip(*finals):
        assert torch.equal(a, b)


def test_loop_wiring_against_the_yardstick_driven_loops(ea):
    """One short update (1 epoch x 4 minibatches, 64 envs x 32 steps, injected RPO noise) three ways from one seed on twin envs:
    kernel, yardstick float32, yardstick float64.  Collection, advantages, permutations and noise are identical (bit for bit);
    with d32 = max |float32-driven - float64-driven| over the parameters, the kernel-driven parameters lie within
    4 x d32 + 1e-7 of the float64-driven ones."""
    import torch
    runs = {}
    for name, dtype in (("kernel", None), ("f32", torch.float32), ("f64", torch.float64)):
        gen = torch.Generator(device=DEV).manual_seed(99)
        alpha = 0.5
        noises = []

        def noise_fn(M, gen=gen, noises=noises):
            z = (torch.rand(M, 2, device=DEV, generator=gen) * 2 - 1) * alpha
            noises.append(z)
            return z
        hooks = {"rpo_noise_fn": noise_fn}
        if dtype is not None:
            hooks["grad_fn"] = _yardstick_grad_fn(dtype, {})
        tr = make_trainer(ea, 10, 64, 32, total_timesteps=64 * 32, num_minibatches=4, update_epochs=1, rpo_alpha=alpha, **hooks)
        tr.update()
        torch.cuda.synchronize()
        runs[name] = SimpleNamespace(params=[p.detach().double().clone() for p in R.mlp_tensors(tr.net)],
                                     storage={k: v.clone() for k, v in tr.storage.items()}, adv=tr.advantages.clone(),
                                     perms=[p.clone() for p in tr.last_permutations], noises=[z.clone() for z in noises])
        tr.env.close()
    k, a, b = runs["kernel"], runs["f32"], runs["f64"]
    for other in (a, b):
        for key in k.storage:
            x, y = k.storage[key], other.storage[key]
            assert torch.equal(x.view(torch.int32), y.view(torch.int32)), key
        assert torch.equal(k.adv, other.adv)
        assert len(k.perms) == 1 and torch.equal(k.perms[0], other.perms[0])
        assert len(k.noises) == 4 and all(torch.equal(x, y) for x, y in zip(k.noises, other.noises))
    d32 = max(float((x - y).abs().max()) for x, y in zip(a.params, b.params))
    dk = max(float((x - y).abs().max()) for x, y in zip(k.params, b.params))
    moved = max(float((x - y.double()).abs().max()) for x, y in zip(b.params, [p.detach() for p in R.mlp_tensors(make_initial_net(6))]))
    print(f"\nloop wiring: d32 = {d32:.3e}, kernel-driven vs float64-driven = {dk:.3e}, bound {4 * d32 + 1e-7:.3e}; the update moved the parameters by {moved:.3e}")
    assert moved > 1e-4                                                       # the update did something
    assert dk <= 4 * d32 + 1e-7, (dk, d32)


def test_the_loop_learns(ea):
    """A smoke test of the loop's sign conventions (N = 10, gravity observation, 256 envs x 128 steps, 4 minibatches x 4 epochs,
    seeded): the mean episodic return of the last 5 of 40 updates exceeds that of the first 5.

    The episodes are cut at 100 steps (``max_timesteps``), below ``num_steps``: every update then records at least 256 finished
    episodes of comparable length.  With the default horizon of 2000 steps the only episodes that finish during the first updates
    are the ones that ended early, whose returns (-1 per step) say how short they were, not how good.  Settled on the
    yardstick-driven loop (float32 yardstick + autograd as ``grad_fn``), never on the kernels: there the mean return rises from
    -85.4 over updates 1-5 to -80.1 over updates 36-40 (256 to 512 episodes per update, every update listed in DESIGN.md
    section 8), so 40 updates separate the two and the update count stays as given."""
    tr = make_trainer(ea, 10, 256, 128, total_timesteps=256 * 128 * 40, num_minibatches=4, update_epochs=4, max_timesteps=100)
    means = []
    for log in tr.learn():
        r = log["episodes"]["episode_reward"]
        assert r.numel() >= 256
        means.append(float(r.mean()))
    tr.env.close()
    print("\nlearning: mean episodic return per update:", " ".join(f"{m:.1f}" for m in means))
    assert len(means) == 40
    first, last = sum(means[:5]) / 5, sum(means[-5:]) / 5
    assert last > first, (first, last)
