"""CPU tests of the deep-sets leader's gradient (include/evac.h: evac_deepsets_workspace_bytes, evac_deepsets_minibatch_grad): the
symbols, every refusal with no device present (no pointer is ever followed: they are made-up addresses), the workspace's size, the
compiled kernels' resources, the yardstick of the GPU tests against the trainer's autograd path, and the entries that keep
refusing a network with a set encoder."""
import ctypes as C
import os
import re

import pytest
import torch

from evacuation_amd import _lib, build
from evacuation_amd.policy import DeepSetsActorCritic, LinearActorCritic
from tests import deepsets_grad_cases as DC
from tests import encoder_grad_cases as G
from tests.encoder_grad_cases import FAKE
from tests.kernel_meta import kernel_resources
from tests.trainer_cases import loss_cfg

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BAD = _lib.ERR_INVALID_ARGUMENT


@pytest.fixture(scope="module")
def lib():
    build.build_library()
    return _lib.load()


def test_symbols_are_declared_exported_and_bound(lib):
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "evac.h")).read(), flags=re.S)
    for name in ("evac_deepsets_workspace_bytes", "evac_deepsets_minibatch_grad"):
        assert re.search(rf"\b{name}\s*\(", text) and name in _lib.SIGNATURES
        getattr(lib, name)
    decl = re.search(r"int evac_deepsets_minibatch_grad\((.*?)\);", text, re.S).group(1)
    assert len(decl.split(",")) == len(lib.evac_deepsets_minibatch_grad.argtypes) == 20
    assert lib.evac_deepsets_workspace_bytes.restype is C.c_int64
    body = re.search(r"typedef struct evac_deepsets_grads \{(.*?)\} evac_deepsets_grads_t;", text, re.S).group(1)
    assert re.findall(r"\*(\w+)", body) == [f for f, _ in _lib.EvacDeepSetsGrads._fields_] == list(DC.ENCODER_NAMES)
    assert C.sizeof(_lib.EvacDeepSetsGrads) == 6 * 8
    assert lib.evac_version() == _lib.VERSION == 150
    assert os.path.join(build.CSRC, "evac_deepsets_train_api.hip") in build.SOURCES


class Call(G.GradCall):
    """A call of evac_deepsets_minibatch_grad whose every argument is acceptable, to be spoiled one argument at a time."""

    def __init__(self, D=36, ed=3, M=4, B=8, norm_adv=1):
        super().__init__(D, M, B, norm_adv)
        self.enc = _lib.EvacDeepSets(ed, 24, *[FAKE] * 6)
        self.enc_grads = _lib.EvacDeepSetsGrads(*[FAKE] * 6)

    def __call__(self, lib):
        return self.grad_call(lib.evac_deepsets_minibatch_grad)


def test_every_refusal_comes_before_a_device_is_touched(lib):
    spoiled = []

    def add(why, **kw):
        c = Call(**kw)
        spoiled.append((why, c))
        return c
    G.rpo_refusals(add, "ed")
    # the encoder's
    add("NULL encoder").null.add("enc")
    add("NULL encoder gradients").null.add("enc_grads")
    for f in DC.ENCODER_NAMES:
        setattr(add(f"NULL encoder.{f}").enc, f, None)
        setattr(add(f"NULL encoder_grads.{f}").enc_grads, f, None)
    add("hidden != 24").enc.hidden = 23
    add("hidden 16").enc.hidden = 16
    add("set_elem_dim 0").enc.set_elem_dim = 0
    add("set_elem_dim 5, which does not divide obs_dim", D=36, ed=5)
    add("set_elem_dim 7", D=42, ed=7)
    add("obs_dim no multiple of set_elem_dim", D=37, ed=3)
    add("fewer than 3 rows", D=12, ed=6)
    add("misaligned rho_w").enc.rho_w = FAKE + 4
    assert len(spoiled) >= 60
    for why, c in spoiled:
        assert c(lib) == BAD, why
    assert Call(M=1, norm_adv=0).cfg.norm_adv == 0   # (one sample without norm_adv is no refusal: not called, nothing to run it on)


def test_workspace_bytes(lib):
    f, g = lib.evac_deepsets_workspace_bytes, lib.evac_rpo_workspace_bytes
    for D in (1, 6, 36, 124, 372, 396):
        prev = 0
        for M in (1, 2, 63, 64, 65, 1000, 4096, 16384, 20000, 100000, (1 << 31) - 1):
            n = f(D, M)
            assert n >= g(D, M) > 0 and n >= prev and n % 16 == 0, (D, M, n)
            # Y and dY, s and t, the gathered columns and the index vector all fit
            assert n >= g(D, M) + M * (2 * D + 2 * 24 + 6) * 4 + M * 8
            prev = n
    for D, M in ((0, 64), (397, 64), (-1, 64), (36, 0), (36, -5), (36, 1 << 31)):
        assert f(D, M) == BAD and g(D, M) == BAD, (D, M)


def test_new_kernels_use_no_scratch_and_spill_no_vgprs():
    kernels = kernel_resources("evac_deepsets_train_api.hip")
    names = [n.split("(")[0] for n in kernels]
    for stem in ("k_set_encode", "k_set_backward", "k_set_finish", "k_rpo_adv_stats<>", "k_rpo_grad<>", "k_rpo_finish<>"):
        assert sum(stem in n for n in names) == 1, (stem, names)
    assert len(kernels) == 6, names
    for name, k in kernels.items():
        assert k["private_segment_fixed_size"] == 0 and k["vgpr_spill_count"] == 0, (name, k)
    assert len(kernel_resources("evac_train_api.hip")) == 8            # evac_train_api.hip's own kernels are as they were


CPU_CASES = [(10, 3, 64, "strided", 1, 1, 0.01, 0.5), (5, 6, 200, "repeat", 0, 0, 0.0, 0.0), (12, 2, 64, "repeat", 1, 0, 0.0, 0.5)]


@pytest.mark.parametrize("N,ed,M,mode,norm_adv,clip_vloss,ent,alpha", CPU_CASES)
def test_the_yardstick_agrees_with_the_trainers_autograd_path(N, ed, M, mode, norm_adv, clip_vloss, ent, alpha):
    """The float32 yardstick (written out from tests/trainer_ref.py and tests/deepsets_ref.py) and autograd_minibatch_grad (the
    module itself) are the same function: both within 4 x the yardstick's own float32-against-float64 error of float64."""
    from evacuation_amd import trainer
    from tests.test_gpu_trainer import stat_errors, tensor_errors
    cfg = loss_cfg(norm_adv, clip_vloss, ent, alpha)
    net, batch, inds, z, g64, s64, t = DC.build_case(N, ed, M, mode, cfg, seed=N + M, device="cpu")
    assert 0.2 <= t.relu_on <= 0.8
    g32, s32, _ = DC.minibatch_grad(net, batch, inds, cfg, z)
    stats = torch.zeros(8)
    trainer.autograd_minibatch_grad(DC.fake_trainer(net, cfg), batch, inds, z, 0, stats)
    ga = [p.grad.clone() for p in DC.all_tensors(net)]
    assert len(ga) == len(g64) == 19
    e32, ea_ = tensor_errors(g32, g64), tensor_errors(ga, g64)
    bound = 4 * max(e32) + 1e-7
    for name, e in zip(DC.NAMES, ea_):
        assert e <= bound, (name, e, bound)
    sbound = 4 * max(stat_errors(s32, s64)) + 1e-7
    for name, e in zip(DC.R.STATS, stat_errors(stats, s64)):
        assert e <= sbound, (name, e, sbound)
    assert all(float(g.abs().max()) > 0 for g in g64[13:])                # the encoder's gradients are there


def test_build_case_clears_the_relu_margin():
    cfg = loss_cfg(1, 1, 0.0, 0.5)
    net, batch, inds, *_ = DC.build_case(64, 6, 500, "strided", cfg, seed=3, device="cpu", cache=False)
    P = [p.detach().double() for p in DC.all_tensors(net)]
    a = DC.preact(P, batch["b_obs"].double())
    assert a.shape == (1003, 66, 24) and float(a.abs().min()) >= DC.RELU_MARGIN


def test_the_linear_entries_keep_refusing_a_set_encoder():
    from evacuation_amd import trainer
    net = DeepSetsActorCritic(36, 10)
    batch = {"b_obs": torch.zeros(8, 36)}
    with pytest.raises(ValueError, match="set encoder"):
        trainer.rpo_minibatch_grad(net, batch, torch.zeros(4, dtype=torch.int64), loss_cfg())
    env = type("Env", (), {"num_envs": 3})()
    with pytest.raises(ValueError, match="set encoder"):
        trainer.RPOTrainer(env, net, trainer.RPOTrainingConfig(), optimizer="device")
    with pytest.raises(ValueError, match="no set encoder"):
        trainer.deepsets_minibatch_grad(LinearActorCritic(6), batch, torch.zeros(4, dtype=torch.int64), loss_cfg())
    assert trainer.RPOTrainer.__init__.__kwdefaults__["grad_fn"] is None and callable(trainer.deepsets_kernel_grad)
