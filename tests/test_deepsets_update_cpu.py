"""CPU tests of the deep-sets leader's optimiser step and whole update (include/evac.h: evac_deepsets_adam_step,
evac_deepsets_minibatch_step, evac_deepsets_update): the symbols, every refusal with no device present (no pointer is ever
followed: they are made-up addresses), the compiled kernels of the new translation unit, the yardstick of the GPU tests over the
19 tensors against torch's own clip + Adam in float64, and the Python entries' argument errors."""
import ctypes as C
import os
import re
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from evacuation_amd import _lib, build
from evacuation_amd.policy import DeepSetsActorCritic, LinearActorCritic, all_tensors
from tests import deepsets_grad_cases as DC
from tests import encoder_grad_cases as G
from tests.encoder_grad_cases import BATCH, FAKE
from tests.kernel_meta import kernel_resources
from tests.optimizer_ref import AdamRef

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BAD = _lib.ERR_INVALID_ARGUMENT
ENTRIES = ("evac_deepsets_adam_step", "evac_deepsets_minibatch_step", "evac_deepsets_update")


@pytest.fixture(scope="module")
def lib():
    build.build_library()
    return _lib.load()


def test_symbols_are_declared_exported_and_bound(lib):
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "evac.h")).read(), flags=re.S)
    counts = {}
    for name in ENTRIES + ("evac_deepsets_minibatch_grad", "evac_adam_step", "evac_rpo_update"):
        decl = re.search(rf"int {name}\((.*?)\);", text, re.S)
        assert decl and name in _lib.SIGNATURES, name
        fn = getattr(lib, name)
        counts[name] = len(decl.group(1).split(","))
        assert len(fn.argtypes) == counts[name] and fn.restype is C.c_int, name
    assert counts["evac_deepsets_minibatch_step"] == counts["evac_deepsets_minibatch_grad"] + 4 == 24
    assert counts["evac_deepsets_adam_step"] == counts["evac_adam_step"] + 3              # the encoder's parameters, gradients, set_elem_dim
    assert counts["evac_deepsets_update"] == counts["evac_rpo_update"] + 3               # the encoder, its parameters, its gradients
    body = re.search(r"typedef struct evac_deepsets_adam_state \{(.*?)\} evac_deepsets_adam_state_t;", text, re.S).group(1)
    assert re.findall(r"(\w+)[,;]", body) == [f for f, _ in _lib.EvacDeepSetsAdamState._fields_] == \
        ["header", "exp_avg", "exp_avg_sq", "enc_exp_avg", "enc_exp_avg_sq"]
    assert C.sizeof(_lib.EvacDeepSetsAdamState) == 8 + 2 * 13 * 8 + 2 * 6 * 8
    assert lib.evac_version() == _lib.VERSION == 150
    assert os.path.join(build.CSRC, "evac_deepsets_update_api.hip") in build.SOURCES


# ------------------------------------------------------------------------------------------------ refusals
class Call(G.GradCall):
    """A call of one of the three entries whose every argument is acceptable, to be spoiled one argument at a time (the pattern of
    tests/test_deepsets_grad_cpu.py)."""

    def __init__(self, entry, D=36, ed=3, M=4, B=8, norm_adv=1, epochs=2):
        super().__init__(D, M, B, norm_adv)
        self.entry = entry
        self.enc = _lib.EvacDeepSets(ed, 24, *[FAKE] * 6)
        self.enc_grads = _lib.EvacDeepSetsGrads(*[FAKE] * 6)
        self.params = _lib.EvacMlpPolicyGrads(*[FAKE] * 13)
        self.enc_params = _lib.EvacDeepSetsGrads(*[FAKE] * 6)
        self.state = _lib.EvacDeepSetsAdamState(FAKE, _lib.EvacMlpPolicyGrads(*[FAKE] * 13), _lib.EvacMlpPolicyGrads(*[FAKE] * 13),
                                                _lib.EvacDeepSetsGrads(*[FAKE] * 6), _lib.EvacDeepSetsGrads(*[FAKE] * 6))
        self.adam = _lib.EvacAdamConfig(3e-4, 0.9, 0.999, 1e-5, 0.5)
        self.D, self.ed, self.epochs = D, ed, epochs
        self.ptr["sumsq"] = FAKE

    def __call__(self, lib):
        ref, p = self.ref, self.ptr
        batch = [self.B] + [p[k] for k in BATCH]
        if self.entry == "evac_deepsets_adam_step":
            return lib.evac_deepsets_adam_step(ref("params"), ref("enc_params"), ref("grads"), ref("enc_grads"), ref("state"), ref("adam"),
                                               self.D, self.ed, p["sumsq"], None)
        if self.entry == "evac_deepsets_minibatch_step":
            return self.grad_call(lib.evac_deepsets_minibatch_step, ref("params"), ref("enc_params"), ref("state"), ref("adam"))
        return lib.evac_deepsets_update(ref("pol"), ref("enc"), ref("params"), ref("enc_params"), ref("grads"), ref("enc_grads"), ref("cfg"),
                                        ref("adam"), ref("state"), *batch, self.M, self.epochs, p["mb_inds"], None, 1, 2, 1, 0.01,
                                        p["stats"], p["workspace"], None)


BAD_ADAM = [("lr", float("nan")), ("lr", float("inf")), ("lr", -float("inf")), ("beta1", -0.1), ("beta1", 1.0), ("beta1", float("nan")),
            ("beta2", -1e-9), ("beta2", 1.0), ("beta2", 1.5), ("eps", 0.0), ("eps", -1e-5), ("eps", float("nan")),
            ("max_grad_norm", 0.0), ("max_grad_norm", -0.5), ("max_grad_norm", float("nan"))]
MLP_FIELDS = [f for f, _ in _lib.EvacMlpPolicyGrads._fields_]


def spoiled_calls(entry):
    spoiled = []

    def add(why, **kw):
        c = Call(entry, **kw)
        spoiled.append((why, c))
        return c
    # what evac_adam_step refuses, and the encoder's part of the optimiser
    for s in ("params", "enc_params", "grads", "enc_grads", "state", "adam"):
        add(f"NULL {s}").null.add(s)
    for f in MLP_FIELDS:
        setattr(add(f"NULL params.{f}").params, f, None)
        setattr(add(f"NULL grads.{f}").grads, f, None)
        setattr(add(f"NULL exp_avg.{f}").state.exp_avg, f, None)
        setattr(add(f"NULL exp_avg_sq.{f}").state.exp_avg_sq, f, None)
    for f in DC.ENCODER_NAMES:
        setattr(add(f"NULL enc_params.{f}").enc_params, f, None)
        setattr(add(f"NULL enc_grads.{f}").enc_grads, f, None)
        setattr(add(f"NULL enc_exp_avg.{f}").state.enc_exp_avg, f, None)
        setattr(add(f"NULL enc_exp_avg_sq.{f}").state.enc_exp_avg_sq, f, None)
    add("NULL header").state.header = None
    add("misaligned header").state.header = FAKE + 4
    for f, v in BAD_ADAM:
        setattr(add(f"{f} = {v}").adam, f, v)
    add("obs_dim 0", D=0)
    add("obs_dim 397", D=397, ed=1)
    add("set_elem_dim 0", ed=0)
    add("set_elem_dim 5, which does not divide obs_dim", D=36, ed=5)
    add("set_elem_dim 7", D=42, ed=7)
    add("obs_dim no multiple of set_elem_dim", D=37, ed=3)
    add("fewer than 3 rows", D=12, ed=6)
    if entry == "evac_deepsets_adam_step":
        add("NULL grad_sumsq").ptr["sumsq"] = None
        return spoiled
    # everything evac_deepsets_minibatch_grad refuses (rpo_prepare's, then the encoder's)
    G.rpo_refusals(add, "ed", own_grads=False)
    add("NULL enc").null.add("enc")
    for f in DC.ENCODER_NAMES:
        setattr(add(f"NULL encoder.{f}").enc, f, None)
    add("encoder hidden != 24").enc.hidden = 23
    add("encoder hidden 16").enc.hidden = 16
    add("misaligned rho_w").enc.rho_w = FAKE + 4
    add("the encoder's set_elem_dim differs: 0").enc.set_elem_dim = 0
    if entry == "evac_deepsets_update":
        add("n_epochs 0", epochs=0)
        add("n_epochs -1", epochs=-1)
    return spoiled


@pytest.mark.parametrize("entry,least", [("evac_deepsets_adam_step", 60), ("evac_deepsets_minibatch_step", 60 + 15 + 8),
                                         ("evac_deepsets_update", 60 + 15 + 8 + 1)])
def test_every_refusal_comes_before_a_device_is_touched(lib, entry, least):
    """At least as many spoiled calls as tests/test_deepsets_grad_cpu.py makes of the gradient (60), and for the step and the
    update the Adam configuration's 15, the header's 2, the moments' and (the update) n_epochs = 0 on top."""
    spoiled = spoiled_calls(entry)
    assert len(spoiled) >= least, len(spoiled)
    assert len({why for why, _ in spoiled}) == len(spoiled)
    for why, c in spoiled:
        assert c(lib) == BAD, (entry, why)


# ------------------------------------------------------------------------------------------------ the compiled kernels
GATED = "<evac::AdamHeader const*>"
# what tests/test_optimizer_cpu.py compares between k_rpo_*<> and their gated twins: the gate costs no vector register, no spill
# and no scratch.  (The highest SCALAR register number is the allocator's numbering, not pressure: the gate's address is one SGPR
# pair that is dead before the first argument is loaded.  k_set_finish's gated twin reports 64 where the plain one reports 62.)
TWIN_FIELDS = ("vgpr_count", "vgpr_spill_count", "sgpr_spill_count", "private_segment_fixed_size")


def test_kernels_of_the_new_unit():
    """evac_deepsets_update_api.hip holds k_adam_set once and the six gradient kernels twice: plain (the step's) and gated by the
    optimiser's header (the update's).  k_adam_set: no scratch, nothing spilled, at most 128 VGPRs; a gated instantiation has its
    plain twin's figures."""
    kernels = kernel_resources("evac_deepsets_update_api.hip")
    by_stem = {}
    for name, k in kernels.items():
        stem = re.sub(r"^void ", "", name.split("(")[0]).replace("evac::", "", 1)
        assert stem not in by_stem, name
        by_stem[stem] = k
    grads = [s + t for s in ("k_set_encode", "k_set_backward", "k_set_finish", "k_rpo_adv_stats", "k_rpo_grad", "k_rpo_finish")
             for t in ("<>", GATED)]
    assert sorted(by_stem) == sorted(["k_adam_set"] + grads), sorted(by_stem)
    adam = by_stem["k_adam_set"]
    print("\nk_adam_set:", adam)
    assert adam["private_segment_fixed_size"] == 0 and adam["vgpr_spill_count"] == 0 and adam["sgpr_spill_count"] == 0, adam
    assert adam["vgpr_count"] <= 128, adam
    for stem in grads:
        k = by_stem[stem]
        assert k["private_segment_fixed_size"] == 0 and k["vgpr_spill_count"] == 0, (stem, k)
        if stem.endswith(GATED):
            plain = by_stem[stem.replace(GATED, "<>")]
            print(stem, k, "| plain:", plain)
            for f in TWIN_FIELDS:
                assert k[f] == plain[f], (stem, f, k, plain)
    # the gradient unit's own kernels, under their names: the plain instantiations
    assert sorted(re.sub(r"^void ", "", n.split("(")[0]).replace("evac::", "", 1) for n in kernel_resources("evac_deepsets_train_api.hip")) == \
        sorted(s for s in grads if s.endswith("<>"))


# ------------------------------------------------------------------------------------------------ the yardstick over 19 tensors
def test_the_yardstick_over_19_tensors_in_float64_is_torch_adam():
    """AdamRef (tests/optimizer_ref.py) over the 19 tensors of N = 10, ed = 3 in float64 against clip_grad_norm_ +
    torch.optim.Adam(eps=1e-5): 10 steps, gradients of four scales (both branches of the clip), an annealed learning rate; the
    bound of tests/test_optimizer_cpu.py::test_the_yardstick_in_float64_is_torch_adam."""
    net = DC.make_net(10, 3, seed=4, device="cpu")
    shapes = [tuple(p.shape) for p in all_tensors(net)]
    assert len(shapes) == 19 and shapes[13:] == [(24, 3), (24,), (24, 24), (24,), (36, 24), (36,)]
    g = torch.Generator().manual_seed(19)
    start = [p.detach().double().clone() for p in all_tensors(net)]
    ps = [p.clone().requires_grad_(True) for p in start]
    opt = torch.optim.Adam(ps, lr=3e-4, eps=1e-5)
    ref_ps = [p.numpy().copy() for p in start]
    ref = AdamRef(ref_ps, np.float64, lr=3e-4, eps=1e-5, max_grad_norm=0.5)
    clipped = 0
    for k in range(10):
        lr = 3e-4 * (1.0 - k / 10)
        grads = [(10.0, 1.0, 1e-3, 1e-5)[k % 4] * torch.randn(*s, generator=g, dtype=torch.float64) for s in shapes]
        opt.param_groups[0]["lr"] = ref.lr = lr
        for p, gr in zip(ps, grads):
            p.grad = gr.clone()
        clipped += int(float(torch.nn.utils.clip_grad_norm_(ps, 0.5)) > 0.5)
        opt.step()
        ref.step(ref_ps, [gr.numpy().copy() for gr in grads])
        d = max(float((p.detach() - torch.from_numpy(r)).abs().max()) for p, r in zip(ps, ref_ps))
        assert d <= 1e-14, (k, d)
    assert 3 <= clipped <= 7 and ref.t == 10
    assert max(float((p.detach() - s).abs().max()) for p, s in zip(ps, start)) > 1e-4


# ------------------------------------------------------------------------------------------------ Python argument errors
def test_python_argument_errors_without_a_device():
    from evacuation_amd import trainer
    deep, linear = DeepSetsActorCritic(36, 10), LinearActorCritic(36)
    with pytest.raises(ValueError, match="contiguous float32 device tensors"):
        trainer.DeviceAdam(deep)
    header, moments = torch.zeros(8, dtype=torch.int64), [torch.zeros_like(p) for p in all_tensors(deep)[:13]]
    with pytest.raises(ValueError, match="storage.*13 tensors"):
        trainer.DeviceAdam(deep, storage=(header, moments, moments))
    cfg = trainer.RPOTrainingConfig(num_envs=4, num_steps=8, num_minibatches=2)
    batch = {"b_obs": torch.zeros(8, 36)}
    inds, perms = torch.arange(4), torch.arange(8)[None]
    opt = object.__new__(trainer.DeviceAdam)                                  # (a DeviceAdam needs a device: one of another network)
    opt.net = DeepSetsActorCritic(36, 10)
    for fn, arg in ((trainer.deepsets_minibatch_step, inds), (trainer.deepsets_update, perms)):
        with pytest.raises(ValueError, match="no set encoder"):
            fn(linear, batch, arg, cfg, opt)
        with pytest.raises(ValueError, match="made for another network"):
            fn(deep, batch, arg, cfg, opt)
        with pytest.raises(TypeError, match="expected a DeviceAdam"):
            fn(deep, batch, arg, cfg, SimpleNamespace(net=deep))
    # the linear entries keep refusing such a network, and the trainer's default gradient with the device optimiser too
    opt.net = deep
    with pytest.raises(ValueError, match="gradient and optimiser kernels are the linear network's"):
        trainer.rpo_minibatch_step(deep, batch, inds, cfg, opt)
    with pytest.raises(ValueError, match="gradient and optimiser kernels are the linear network's"):
        trainer.RPOTrainer(SimpleNamespace(num_envs=4), deep, cfg, optimizer="device")
