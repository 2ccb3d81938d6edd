"""CPU checks of the optimiser step (evac_adam_step, evac_rpo_minibatch_step, evac_rpo_update; DeviceAdam): the entries are
exported and bound and refuse bad arguments on the host with no GPU present; the NumPy statement of the step
(tests/optimizer_ref.py) IS clip_grad_norm_ + torch.optim.Adam(eps=1e-5) in float64, and in float32 it is as accurate as torch's
own float32 Adam; the new kernels use no scratch and spill nothing."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch

from evacuation_amd import _lib, build
from tests.kernel_meta import kernel_resources
from tests.optimizer_ref import AdamRef

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BAD = _lib.ERR_INVALID_ARGUMENT
P = 0x1000                           # a non-NULL, 16-byte aligned address that is never followed


@pytest.fixture(scope="module")
def lib():
    build.build_library()
    return _lib.load()


def declared_arg_counts():
    text = open(os.path.join(ROOT, "include", "evac.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    out = {}
    for name, args in re.findall(r"\b(evac_[a-z_0-9]+)\s*\(([^;{}]*?)\)\s*;", text, flags=re.S):
        out[name] = 0 if args.strip() in ("", "void") else args.count(",") + 1
    return out


def test_optimizer_symbols_are_exported_and_bound(lib):
    counts = declared_arg_counts()
    for name in ("evac_adam_step", "evac_rpo_minibatch_step", "evac_rpo_update"):
        assert name in _lib.SIGNATURES
        fn = getattr(lib, name)
        assert len(fn.argtypes) == counts[name], (name, len(fn.argtypes), counts[name])
        assert fn.restype is C.c_int
    assert counts["evac_adam_step"] == 7
    assert counts["evac_rpo_minibatch_step"] == counts["evac_rpo_minibatch_grad"] + 3
    assert counts["evac_rpo_minibatch_grad"] == len(lib.evac_rpo_minibatch_grad.argtypes)      # the parser itself, on an old entry
    assert C.sizeof(_lib.EvacAdamConfig) == 40 and C.sizeof(_lib.EvacAdamState) == 8 + 2 * 104
    assert [f for f, _ in _lib.EvacAdamConfig._fields_] == ["lr", "beta1", "beta2", "eps", "max_grad_norm"]
    assert lib.evac_version() == 150


def _tensors(n_null=None):
    t = [P] * 13
    if n_null is not None:
        t[n_null] = None
    return _lib.EvacMlpPolicyGrads(*t)


def _state(header=P, m=None, v=None):
    return _lib.EvacAdamState(header, m or _tensors(), v or _tensors())


def _adam(lr=3e-4, b1=0.9, b2=0.999, eps=1e-5, clip=0.5):
    return _lib.EvacAdamConfig(lr, b1, b2, eps, clip)


BAD_ADAM = [dict(lr=float("nan")), dict(lr=float("inf")), dict(lr=-float("inf")), dict(b1=-0.1), dict(b1=1.0), dict(b1=float("nan")),
            dict(b2=-1e-9), dict(b2=1.0), dict(b2=1.5), dict(eps=0.0), dict(eps=-1e-5), dict(eps=float("nan")), dict(clip=0.0),
            dict(clip=-0.5), dict(clip=float("nan"))]


def test_adam_step_validation_needs_no_gpu(lib):
    """Every refusal comes before anything touches a device (the pointers here are never followed)."""
    def call(params=None, grads=None, state=None, cfg=None, D=6, sumsq=P, null=None):
        args = [C.byref(params or _tensors()), C.byref(grads or _tensors()), C.byref(state or _state()), C.byref(cfg or _adam()), D, sumsq, None]
        if null is not None:
            args[null] = None
        return lib.evac_adam_step(*args)

    for i in (0, 1, 2, 3, 5):
        assert call(null=i) == BAD, i
    for D in (0, -1, 397):
        assert call(D=D) == BAD, D
    for i in (0, 6, 12):
        assert call(params=_tensors(i)) == BAD and call(grads=_tensors(i)) == BAD
        assert call(state=_state(m=_tensors(i))) == BAD and call(state=_state(v=_tensors(i))) == BAD
    assert call(state=_state(header=None)) == BAD and call(state=_state(header=P + 4)) == BAD     # 8-byte alignment
    for kw in BAD_ADAM:
        assert call(cfg=_adam(**kw)) == BAD, kw


def test_minibatch_step_and_update_validation_needs_no_gpu(lib):
    pol_ok = lambda: _lib.EvacMlpPolicy(6, 64, *([P] * 13))
    loss_ok = lambda norm_adv=1: _lib.EvacRpoLossConfig(0.2, 0.0, 0.5, 0.5, norm_adv, 1)

    def step(pol=None, loss=None, B=128, ptrs=None, M=64, inds=P, grads=None, stats=P, ws=P, params=None, state=None, cfg=None, null=()):
        keep = [pol or pol_ok(), loss or loss_ok(), grads or _tensors(), params or _tensors(), state or _state(), cfg or _adam()]
        args = [C.byref(keep[0]), C.byref(keep[1]), B, *(ptrs or [P] * 6), M, inds, None, 0, 0, C.byref(keep[2]), stats, ws, None,
                C.byref(keep[3]), C.byref(keep[4]), C.byref(keep[5])]
        for i in null:
            args[i] = None
        return lib.evac_rpo_minibatch_step(*args)

    def update(pol=None, params=None, grads=None, loss=None, cfg=None, state=None, B=128, ptrs=None, M=64, epochs=3, perms=P, stats=P,
               ws=P, null=()):
        keep = [pol or pol_ok(), params or _tensors(), grads or _tensors(), loss or loss_ok(), cfg or _adam(), state or _state()]
        args = [C.byref(k) for k in keep] + [B, *(ptrs or [P] * 6), M, epochs, perms, None, 0, 0, 1, 0.01, stats, ws, None]
        for i in null:
            args[i] = None
        return lib.evac_rpo_update(*args)

    # NULL pointers (rpo_noise and the stream excepted)
    for i in (0, 1, 14, 18, 19, 20):
        assert step(null=(i,)) == BAD, i
    for i in range(6):
        assert update(null=(i,)) == BAD, i
    for i in range(6):
        ptrs = [P] * 6
        ptrs[i] = None
        assert step(ptrs=ptrs) == BAD and update(ptrs=ptrs) == BAD, i
    assert step(inds=None) == BAD and step(stats=None) == BAD and step(ws=None) == BAD and step(ws=P + 4) == BAD
    assert update(perms=None) == BAD and update(stats=None) == BAD and update(ws=None) == BAD and update(ws=P + 8) == BAD
    for fn in (step, update):
        assert fn(pol=_lib.EvacMlpPolicy(6, 32, *([P] * 13))) == BAD                        # hidden != 64
        assert fn(pol=_lib.EvacMlpPolicy(0, 64, *([P] * 13))) == BAD and fn(pol=_lib.EvacMlpPolicy(397, 64, *([P] * 13))) == BAD
        assert fn(pol=_lib.EvacMlpPolicy(6, 64, *([P] * 12 + [None]))) == BAD
        assert fn(grads=_tensors(0)) == BAD and fn(params=_tensors(12)) == BAD
        assert fn(state=_state(header=None)) == BAD and fn(state=_state(header=P + 4)) == BAD
        assert fn(state=_state(m=_tensors(3))) == BAD and fn(state=_state(v=_tensors(7))) == BAD
        assert fn(B=0) == BAD and fn(B=-1) == BAD and fn(M=0) == BAD and fn(M=-5) == BAD
        assert fn(M=1) == BAD                                                               # norm_adv: the std of one sample
        for kw in BAD_ADAM:
            assert fn(cfg=_adam(**kw)) == BAD, kw
    assert update(epochs=0) == BAD and update(epochs=-1) == BAD


# ------------------------------------------------------------------------------------------------ the yardstick itself
SHAPES = [(64, 6), (64,), (64, 64), (2, 64), (2,), (1, 2), (1,)]
SCALES = (10.0, 1.0, 1e-3, 1e-5)


def _inputs(steps, seed=0):
    """Start parameters of magnitude about 1 and, per step, gradients of one of four scales (the large ones clip) and an
    annealed learning rate."""
    g = torch.Generator().manual_seed(seed)
    params = [torch.randn(*s, generator=g, dtype=torch.float64) for s in SHAPES]
    grads = []
    for k in range(steps):
        scale = SCALES[k % 4] if k % 8 < 4 else SCALES[int(torch.randint(0, 4, (1,), generator=g))]
        grads.append([scale * torch.randn(*s, generator=g, dtype=torch.float64) for s in SHAPES])
    lrs = [3e-4 * (1.0 - k / steps) for k in range(steps)]
    return params, grads, lrs


def _run_torch(params, grads, lrs, dtype, marks):
    ps = [p.to(dtype).clone().requires_grad_(True) for p in params]
    opt = torch.optim.Adam(ps, lr=3e-4, eps=1e-5)
    out, clipped = {}, 0
    for k, (gs, lr) in enumerate(zip(grads, lrs)):
        opt.param_groups[0]["lr"] = lr
        for p, g in zip(ps, gs):
            p.grad = g.to(dtype).clone()
        norm = torch.nn.utils.clip_grad_norm_(ps, 0.5)
        clipped += int(float(norm) > 0.5)
        opt.step()
        if k + 1 in marks:
            out[k + 1] = [p.detach().double().clone() for p in ps]
    return out, clipped


def _run_ref(params, grads, lrs, dtype, marks):
    ps = [p.numpy().astype(dtype) for p in params]
    opt = AdamRef(ps, dtype=dtype, lr=3e-4, eps=1e-5, max_grad_norm=0.5)
    out = {}
    for k, (gs, lr) in enumerate(zip(grads, lrs)):
        opt.lr = lr
        opt.step(ps, [g.numpy().astype(dtype) for g in gs])
        if k + 1 in marks:
            out[k + 1] = [torch.from_numpy(p.astype(np.float64)) for p in ps]
    rel = opt.t * 2.0 ** -52                                                  # one rounding per product at most (and pow's own)
    assert opt.t == len(lrs) and abs(opt.P1 - 0.9 ** opt.t) <= rel * 0.9 ** opt.t and abs(opt.P2 - 0.999 ** opt.t) <= rel * 0.999 ** opt.t
    return out


def _maxdiff(a, b):
    return max(float((x - y).abs().max()) for x, y in zip(a, b))


MARKS = (1, 10, 320, 1000, 2000)


@pytest.fixture(scope="module")
def runs():
    params, grads, lrs = _inputs(2000)
    t64, clipped = _run_torch(params, grads, lrs, torch.float64, MARKS)
    assert 600 <= clipped <= 1400, clipped                                    # both branches of the clip, each many times
    return {"t64": t64, "t32": _run_torch(params, grads, lrs, torch.float32, MARKS)[0],
            "r64": _run_ref(params, grads, lrs, np.float64, MARKS), "r32": _run_ref(params, grads, lrs, np.float32, MARKS)}


def test_the_yardstick_in_float64_is_torch_adam(runs):
    """Parameters of magnitude about 1: 1e-14 absolute is ten times what was measured (8.9e-16 after 2000 steps) and nine orders
    below float32."""
    for k in MARKS:
        d = _maxdiff(runs["r64"][k], runs["t64"][k])
        print(f"\nfloat64 yardstick vs torch float64 after {k} steps: {d:.2e}")
        assert d <= 1e-14, (k, d)
    assert _maxdiff(runs["t64"][2000], runs["t64"][1]) > 1e-2                 # the run moved the parameters


def test_the_yardstick_in_float32_is_as_accurate_as_torch(runs):
    for k in MARKS:
        e_ref, e_torch = _maxdiff(runs["r32"][k], runs["t64"][k]), _maxdiff(runs["t32"][k], runs["t64"][k])
        print(f"\nafter {k} steps: float32 yardstick {e_ref:.2e}, torch float32 {e_torch:.2e} (against torch float64)")
        assert e_ref <= 4 * e_torch + 1e-7, (k, e_ref, e_torch)


def test_the_yardstick_keeps_a_nan_and_counts_without_the_host():
    ps = [np.ones(4, np.float32)]
    opt = AdamRef(ps, np.float32)
    opt.step(ps, [np.array([1.0, np.nan, 0.0, 2.0], np.float32)])
    assert np.isnan(ps[0]).all() and np.isnan(opt.last_clip_coef)
    assert opt.clip_coef(np.float32(100.0)) == np.float32(0.5) / (np.float32(10.0) + np.float32(1e-6))
    assert opt.clip_coef(np.float32(0.01)) == 1.0 and opt.clip_coef(np.float32(0.0)) == 1.0


# ------------------------------------------------------------------------------------------------ the compiled kernels
def test_new_kernels_use_no_scratch_and_spill_nothing():
    """From the compiled device code, as test_kernel_resource_budgets reads it: k_adam and the stop-aware instantiations of the
    gradient kernels."""
    by_name = {n: {f: k[f] for f in ("vgpr_count", "vgpr_spill_count", "sgpr_spill_count", "private_segment_fixed_size")}
               for n, k in kernel_resources("evac_train_api.hip").items()}
    stems = ["k_gae", "k_adam"] + [s + t for s in ("k_rpo_adv_stats", "k_rpo_grad", "k_rpo_finish") for t in ("<>", "<evac::AdamHeader const*>")]
    assert len(by_name) == 8 and all(sum(s in n for n in by_name) == 1 for s in stems), list(by_name)      # these eight and no other
    adam = [k for n, k in by_name.items() if "k_adam" in n]
    assert len(adam) == 1
    assert adam[0]["private_segment_fixed_size"] == 0 and adam[0]["vgpr_spill_count"] == 0 and adam[0]["sgpr_spill_count"] == 0, adam
    assert adam[0]["vgpr_count"] <= 128, adam
    for stem in ("k_rpo_adv_stats", "k_rpo_grad", "k_rpo_finish"):
        plain = [k for n, k in by_name.items() if stem + "<>" in n]
        gated = [k for n, k in by_name.items() if stem + "<" in n and "AdamHeader" in n]
        assert len(plain) == 1 and len(gated) == 1, (stem, list(by_name))
        assert gated[0]["private_segment_fixed_size"] == 0 and gated[0]["vgpr_spill_count"] == 0, (stem, gated)
        assert gated[0] == plain[0], (stem, plain, gated)                      # the gate costs no register and no spill
    assert not any(t in n for n in by_name if "k_adam" in n or "k_rpo" in n for t in ("k_step", "k_rollout", "k_reset", "k_observe"))


# ------------------------------------------------------------------------------------------------ argument errors of the Python face
def test_python_argument_errors_need_no_device():
    from evacuation_amd.policy import LinearActorCritic
    from evacuation_amd.trainer import DeviceAdam, RPOTrainer, RPOTrainingConfig
    net = LinearActorCritic(6)
    for kw in (dict(lr=float("nan")), dict(lr=float("inf")), dict(betas=(1.0, 0.999)), dict(betas=(0.9, -0.1)), dict(eps=0.0),
               dict(max_grad_norm=0.0), dict(max_grad_norm=-1.0)):
        with pytest.raises(ValueError):
            DeviceAdam(net, **kw)
    with pytest.raises(ValueError, match="device tensors"):
        DeviceAdam(net)                                                        # a CPU network: there is no CPU fallback

    class Env:
        num_envs = 3
    with pytest.raises(ValueError, match="nonsense"):
        RPOTrainer(Env(), net, RPOTrainingConfig(), optimizer="nonsense")
    import evacuation_amd
    assert evacuation_amd.DeviceAdam is DeviceAdam and callable(evacuation_amd.rpo_minibatch_step) and callable(evacuation_amd.rpo_update)
