"""What the gradient tests of the linear network and of the two encoders share: the one branch-covering minibatch recipe
(``build_case``, called by tests/trainer_cases.py, tests/deepsets_grad_cases.py and tests/transformer_grad_cases.py, each with its
own network, redraw rounds, float64 encoding and yardstick) and the bodies of the GPU tests that tests/test_gpu_deepsets_grad.py
and tests/test_gpu_transformer_grad.py run alike, each with a description of its encoder (``Encoder``)."""
import math
import os
import subprocess
import sys
from collections import namedtuple
from types import SimpleNamespace

import pytest

from tests import trainer_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEV = "cuda:0"


def all_tensors(net):
    from evacuation_amd.policy import all_tensors as f
    return f(net)


def fake_trainer(net, cfg):
    return SimpleNamespace(net=net, cfg=cfg)


def kernel_grad_of(entry):
    """``kernel_grad(net, batch, inds, cfg, z, **kw)`` -> (the gradients of all tensors, the statistics) by ``trainer.<entry>``."""
    def kernel_grad(net, batch, inds, cfg, z, **kw):
        import torch
        from evacuation_amd import trainer
        stats = getattr(trainer, entry)(net, batch, inds, cfg, rpo_noise=z, **kw)
        torch.cuda.synchronize()
        return [p.grad.clone() for p in all_tensors(net)], stats.clone()
    return kernel_grad


# ------------------------------------------------------------------------------------------------ the recipe
def draw_obs(rows, D, g):
    import torch
    return (0.6 * torch.randn(rows, D, generator=g)).clamp(-1, 1)


def redraw_rows(obs, g, near):
    """The rows of obs [B, D] that ``near(obs)`` marks (a bool [B]) drawn again from ``g``, in place, at most 8 rounds."""
    for _ in range(8):
        bad = near(obs)
        n = int(bad.sum())
        if n == 0:
            break
        obs[bad] = draw_obs(n, obs.shape[1], g)


_CASES = {}


def build_case(D, M, mode, cfg, seed, device, make_net, encode64, yardstick, key=None):
    """A batch whose minibatch takes every branch of the loss by a known share of its samples: the old log-probabilities and
    values are set FROM the float64 forward pass so that the ratio lies inside the clip range for half of the batch rows, above
    it for a quarter and below it for a quarter (advantages of both signs everywhere), and the value difference likewise around
    +-clip_coef -- each with a margin, so no sample is within 1e-6 of a branch point of max / clamp (checked, regenerated from
    another seed otherwise).  ``mode``: 'repeat' (indices drawn with repetition from a batch of M rows) or 'strided' (every second
    row of a batch of 2 M + 3).

    ``make_net()``: the network, on ``device``.  ``encode64(net, obs, g)``: the builder's redraw rounds on ``obs`` (in place, from
    ``g``: ``redraw_rows``), then (the actor-critic's 13 tensors in float64 on the CPU, what they read for every batch row in
    float64, ``attach`` or None); ``attach(t, batch, inds)`` adds the builder's own figures to the terms.  ``yardstick(net, batch,
    inds, cfg, z, dtype)`` -> (gradients, statistics, terms).  One generator draws inds, obs (and its redraws), act, z, u, mag,
    inside, u2, mag2, inside2, returns, adv, in that order.  ``key``: the builder's part of the key the case is kept under, built
    once per process and shared (nobody changes it); None: not kept.  Returns (net, batch, inds, z, g64, s64, t)."""
    import torch
    if key is not None:
        key += (M, mode, cfg.norm_adv, cfg.clip_vloss, cfg.ent_coef, cfg.rpo_alpha, cfg.clip_coef, cfg.vf_coef, seed, str(device))
        if key in _CASES:
            return _CASES[key]
    c = cfg.clip_coef
    for attempt in range(8):
        g = torch.Generator().manual_seed(seed + 1000 * attempt)
        net = make_net()
        B = max(M, 4) if mode == "repeat" else 2 * M + 3
        inds = torch.randint(0, B, (M,), generator=g) if mode == "repeat" else torch.arange(M) * 2 + 1
        obs = draw_obs(B, D, g)
        P, y64, attach = encode64(net, obs, g)
        act = torch.randn(B, 2, generator=g)
        z = (torch.rand(M, 2, generator=g) * 2 - 1) * cfg.rpo_alpha
        # the float64 forward pass of every batch row, with the perturbation of the LAST minibatch position that reads the row
        zrow = torch.zeros(B, 2)
        zrow[inds] = z
        lp, _, val = R.logprob_entropy_value(P, y64, act.double(), zrow.double())
        u = torch.rand(B, generator=g)
        mag = 0.25 + 0.35 * torch.rand(B, generator=g)                                    # |log ratio| in [0.25, 0.6]: ratio <= 0.78 or >= 1.28
        inside = (0.05 * torch.randn(B, generator=g)).clamp(-0.12, 0.12)
        target = torch.where(u < 0.5, inside, torch.where(u < 0.75, mag, -mag))
        logprobs = (lp - target.double()).float()
        u2 = torch.rand(B, generator=g)
        mag2 = c * (1.25 + torch.rand(B, generator=g))
        inside2 = c * (0.3 * torch.randn(B, generator=g)).clamp(-0.8, 0.8)
        dv = torch.where(u2 < 0.5, inside2, torch.where(u2 < 0.75, mag2, -mag2))
        values = (val.view(-1) - dv.double()).float()
        returns = (val.view(-1) + 0.7 * torch.randn(B, generator=g).double()).float()
        adv = torch.randn(B, generator=g) + 0.3
        batch = {"b_obs": obs, "b_actions": act, "b_logprobs": logprobs, "b_advantages": adv, "b_returns": returns, "b_values": values}
        batch = {k: v.to(device).contiguous() for k, v in batch.items()}
        inds, z = inds.to(device), z.to(device).contiguous()
        g64, s64, t = yardstick(net, batch, inds, cfg, z, torch.float64)
        near = ((t.ratio - (1 - c)).abs() < 1e-6) | ((t.ratio - (1 + c)).abs() < 1e-6) | (t.adv.abs() < 1e-6)
        near |= ((t.dv.abs() - c).abs() < 1e-6)
        if cfg.clip_vloss:
            near |= ((t.dv.abs() > c) & ((t.v_unclipped - t.v_clipped).abs() < 1e-6))
        if not bool(near.any()):
            if attach is not None:
                attach(t, batch, inds)
            out = (net, batch, inds, z, g64, s64, t)
            if key is not None:
                _CASES[key] = out
            return out
    raise AssertionError("could not build a case without samples at a branch point")


# ------------------------------------------------------------------------------------------------ the GPU tests' shared bodies
# An encoder as the bodies below see it: its cases module (all_tensors, minibatch_grad, kernel_grad, R), names(number of tensors),
# tensor_errors(got, g64) with the encoder's own scaling, the names in evacuation_amd.trainer of its gradient entry and of its
# grad_fn, its network's class in evacuation_amd.policy, --network of examples/train_rpo.py, the bound's factor and the width of
# the printed names.
Encoder = namedtuple("Encoder", "cases names tensor_errors entry grad_fn net_class network factor width")


@pytest.fixture(scope="module")
def ea():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("needs an MI355X")
    import evacuation_amd
    return evacuation_amd


def stat_errors(s, s64):
    from tests.test_gpu_trainer import stat_errors as f
    return f(s, s64)


def check_against_float64(enc, gk, sk, g32, s32, g64, s64, title):
    """Every tensor and statistic of the kernel within enc.factor x the float32 yardstick's largest error + 1e-7."""
    names = enc.names(len(g64))
    e32, ek = enc.tensor_errors(g32, g64), enc.tensor_errors(gk, g64)
    se32, sek = stat_errors(s32, s64), stat_errors(sk, s64)
    bound, sbound = enc.factor * max(e32) + 1e-7, enc.factor * max(se32) + 1e-7
    print(f"\n{title}: e32(case) = {max(e32):.2e}, bound {bound:.2e}; statistics e32 = {max(se32):.2e}, bound {sbound:.2e}")
    for name, a, b in zip(names, e32, ek):
        print(f"  {name:{enc.width}s} torch f32 {a:.2e}   kernel {b:.2e}   ratio to e32(case) {b / max(e32):.2f}")
    for name, a, b in zip(R.STATS, se32, sek):
        print(f"  {name:{enc.width}s} torch f32 {a:.2e}   kernel {b:.2e}")
    for name, b in zip(names, ek):
        assert b <= bound, (name, b, bound)
    for name, b in zip(R.STATS, sek):
        assert b <= sbound, (name, b, sbound)


def check_deterministic_and_written_not_accumulated(enc, cfg, net, batch, inds, z):
    import torch
    C = enc.cases
    g1, s1 = C.kernel_grad(net, batch, inds, cfg, z)
    names = enc.names(len(g1))
    for p in C.all_tensors(net):
        p.grad.fill_(7.0)                                                     # written, not accumulated
    junk = [torch.randn(1 << 20, device=DEV) for _ in range(5)]               # unrelated allocations and work
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        g2, s2 = C.kernel_grad(net, batch, inds, cfg, z)
    side.synchronize()
    del junk
    for name, a, b in zip(names, g1, g2):
        assert torch.equal(a, b), name
    assert torch.equal(s1, s2)
    # the perturbation drawn on the device: equal bits for equal (seed, draw_counter), another draw for another counter
    seed, counter = 0x1234567890ABCDEF, (7 << 32) + 5
    gd, sd = C.kernel_grad(net, batch, inds, cfg, None, seed=seed, draw_counter=counter)
    ge, se = C.kernel_grad(net, batch, inds, cfg, None, seed=seed, draw_counter=counter)
    for name, a, b in zip(names, gd, ge):
        assert torch.equal(a, b), name
    assert torch.equal(sd, se)
    _, so = C.kernel_grad(net, batch, inds, cfg, None, seed=seed, draw_counter=counter + 1)
    assert not torch.equal(so, sd)


def check_in_place_contract_under_graph_capture(enc, cfg, net, batch, inds, z):
    """``inds``: 64 indices into a batch of at least 127 rows."""
    import torch
    from evacuation_amd import trainer
    C, minibatch_grad = enc.cases, getattr(trainer, enc.entry)
    stats = torch.zeros(8, device=DEV)
    minibatch_grad(net, batch, inds, cfg, rpo_noise=z, stats=stats)                                   # warm-up: binds, allocates
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        minibatch_grad(net, batch, inds, cfg, rpo_noise=z, stats=stats)
    before = [p.grad.clone() for p in C.all_tensors(net)]
    with torch.no_grad():
        for p in C.all_tensors(net):
            p.add_(0.05 * torch.randn_like(p))                                                        # in place: same addresses
        inds.copy_(torch.arange(64, device=DEV) * 2)                                                  # other rows, same vector
    graph.replay()
    torch.cuda.synchronize()
    replayed = [p.grad.clone() for p in C.all_tensors(net)]
    replayed_stats = stats.clone()
    direct, direct_stats = C.kernel_grad(net, batch, inds, cfg, z)
    for name, a, b, c in zip(enc.names(len(direct)), replayed, direct, before):
        assert torch.equal(a, b), name
        assert not torch.equal(a, c), name
    assert torch.equal(replayed_stats, direct_stats)
    g64, _, _ = C.minibatch_grad(net, batch, inds, cfg, z, torch.float64)                             # ... and they are the new inputs' gradients
    assert max(enc.tensor_errors(replayed, g64)) < 1e-3


def check_trainer_wiring(enc, ea, check_trainer=None):
    """N = 10, the abs + cat Box observation (D = 36), 8 envs x 16 steps, 2 minibatches x 2 epochs: one update() with the encoder's
    ``grad_fn``, every call recorded, replayed bit for bit and held to float64.  ``check_trainer(env, net, cfg)``: the encoder's
    own assertions before the update.  Returns (the tensors before, after, the recorded calls, cfg)."""
    import torch
    from evacuation_amd import policy, trainer
    C = enc.cases
    cfg = trainer.RPOTrainingConfig(seed=3, num_envs=8, num_steps=16, total_timesteps=8 * 16, num_minibatches=2, update_epochs=2)
    env = ea.NormalizedVectorEnv.make(ea.EnvConfig(number_of_pedestrians=10), ea.EnvWrappersConfig(positions="abs", statuses="cat", type="Box"),
                                      num_envs=8, gamma=cfg.gamma, seed=3)
    assert env.obs_dim == 36
    torch.manual_seed(0)
    net = getattr(policy, enc.net_class)(env.obs_dim, 10).to(DEV)
    tensors = C.all_tensors(net)
    names = enc.names(len(tensors))
    initial = [p.detach().clone() for p in tensors]
    gen = torch.Generator(device=DEV).manual_seed(99)
    calls = []

    def grad_fn(tr, batch, mb_inds, rpo_noise, draw_counter, stats):
        params = [p.detach().clone() for p in tensors]
        out = getattr(trainer, enc.grad_fn)(tr, batch, mb_inds, rpo_noise, draw_counter, stats)
        calls.append((params, {k: v.clone() for k, v in batch.items()}, mb_inds.clone(), rpo_noise.clone(), draw_counter,
                      [p.grad.clone() for p in tensors], out.clone()))
        return out
    tr = trainer.RPOTrainer(env, net, cfg, grad_fn=grad_fn,
                            rpo_noise_fn=lambda M: (torch.rand(M, 2, device=DEV, generator=gen) * 2 - 1) * cfg.rpo_alpha)
    assert trainer.RPOTrainer(env, net, cfg).grad_fn is trainer.autograd_minibatch_grad           # the default stays autograd's
    if check_trainer is not None:
        check_trainer(env, net, cfg)
    log = tr.update()
    torch.cuda.synchronize()
    assert len(calls) == 4 and [c[4] for c in calls] == [0, 1, 2, 3]
    assert all(math.isfinite(v) for k, v in log.items() if isinstance(v, float) and k != "explained_variance"), log
    final = [p.detach().clone() for p in tensors]
    assert all(bool(torch.isfinite(b).all()) for b in final)
    for i, (params, batch, mb_inds, noise, counter, grads, stats) in enumerate(calls):
        with torch.no_grad():
            for p, q in zip(tensors, params):
                p.copy_(q)                                                                            # the parameters of that moment
        gd, sd = C.kernel_grad(net, batch, mb_inds, cfg, noise, seed=cfg.seed, draw_counter=counter)
        for name, a, b in zip(names, grads, gd):
            assert torch.equal(a, b), (i, name)
        assert torch.equal(stats, sd)
        g64, s64, _ = C.minibatch_grad(net, batch, mb_inds, cfg, noise, torch.float64)
        g32, s32, _ = C.minibatch_grad(net, batch, mb_inds, cfg, noise)
        check_against_float64(enc, grads, stats, g32, s32, g64, s64, f"trainer wiring, call {i}")
    env.close()
    return initial, final, calls, cfg


def check_train_rpo_example_with_the_device_gradient(enc):
    cmd = [sys.executable, os.path.join(ROOT, "examples", "train_rpo.py"), "--network", enc.network, "--gradient", "device", "--envs", "8",
           "--steps", "16", "--updates", "2", "--pedestrians", "10", "--minibatches", "2", "--epochs", "2"]
    done = subprocess.run(cmd, cwd=ROOT, capture_output=True, text=True, timeout=120)
    assert done.returncode == 0, done.stdout[-2000:] + done.stderr[-2000:]
    assert done.stdout.count("SPS:") == 2, done.stdout[-2000:]


# ------------------------------------------------------------------------------------------------ the CPU tests' refusal tables
FAKE = 0x1000                                    # 16-byte aligned, never followed
BATCH = ("b_obs", "b_actions", "b_logprobs", "b_advantages", "b_returns", "b_values")


class GradCall:
    """A call of an encoder's gradient entry whose every argument is acceptable, to be spoiled one argument at a time: the part
    the entries share.  A subclass adds ``enc`` and ``enc_grads`` (and what its entry takes beside them)."""

    def __init__(self, D, M, B, norm_adv):
        from evacuation_amd import _lib
        self.pol = _lib.EvacMlpPolicy(D, 64, *[FAKE] * 13)
        self.cfg = _lib.EvacRpoLossConfig(0.2, 0.0, 0.5, 0.5, norm_adv, 1)
        self.grads = _lib.EvacMlpPolicyGrads(*[FAKE] * 13)
        self.B, self.M = B, M
        self.ptr = {k: FAKE for k in BATCH + ("mb_inds", "stats", "workspace")}
        self.null = set()                        # structs passed as NULL

    def ref(self, name):
        import ctypes as C
        return None if name in self.null else C.byref(getattr(self, name))

    def grad_call(self, fn, *more):
        """``fn`` with evac_deepsets_minibatch_grad's arguments (no noise, seed 1, draw counter 2, no stream), then ``more``."""
        p = self.ptr
        return fn(self.ref("pol"), self.ref("enc"), self.ref("cfg"), self.B, *[p[k] for k in BATCH], self.M, p["mb_inds"], None, 1, 2,
                  self.ref("grads"), self.ref("enc_grads"), p["stats"], p["workspace"], None, *more)


def rpo_refusals(add, elem, own_grads=True):
    """Everything evac_rpo_minibatch_grad refuses, as rows of a table: ``add(why, **kw)`` makes the call to spoil.  ``elem``: the
    keyword of the encoder's element width (1 goes with any obs_dim).  Without ``own_grads`` the rows that a table with the
    optimiser's refusals has already (the gradients' struct, obs_dim) are left out."""
    from evacuation_amd import _lib
    for s in ("pol", "cfg") + (("grads",) if own_grads else ()):
        add(f"NULL {s}").null.add(s)
    for k in BATCH + ("mb_inds", "stats", "workspace"):
        add(f"NULL {k}").ptr[k] = None
    for f, _ in _lib.EvacMlpPolicy._fields_[2:]:
        setattr(add(f"NULL policy.{f}").pol, f, None)
        if own_grads:
            setattr(add(f"NULL grads.{f}").grads, f, None)
    add("hidden != 64").pol.hidden = 32
    if own_grads:
        add("obs_dim 0").pol.obs_dim = 0
        add("obs_dim 397", D=397, **{elem: 1})
    add("batch_size 0", B=0)
    add("M 0", M=0)
    add("M 2^31", M=1 << 31)
    add("norm_adv with one sample", M=1)
    add("misaligned workspace").ptr["workspace"] = FAKE + 8
