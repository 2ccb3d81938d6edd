"""CPU tests of the transformer leader's gradient (include/evac.h: evac_transformer_workspace_bytes,
evac_transformer_minibatch_grad): the symbols, every refusal with no device present (no pointer is ever followed: they are made-up
addresses) with the code of each cause, the workspace's size, the compiled kernels' resources, the yardstick of the GPU tests
against the trainer's autograd path, the case builder's conditions, and what stays as it was for such a network."""
import ctypes as C
import os
import re
import subprocess
import tempfile
from types import SimpleNamespace

import pytest
import torch

from evacuation_amd import _lib, build
from evacuation_amd.policy import _BLOCK_TENSORS, LinearActorCritic, TransformerActorCritic
from tests import encoder_grad_cases as G
from tests import transformer_grad_cases as TC
from tests.encoder_grad_cases import FAKE
from tests.kernel_meta import kernel_resources
from tests.trainer_cases import loss_cfg

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BAD, UNSUPPORTED = _lib.ERR_INVALID_ARGUMENT, _lib.ERR_UNSUPPORTED
UNIT = "evac_transformer_train_api.hip"


@pytest.fixture(scope="module")
def lib():
    build.build_library()
    return _lib.load()


def test_symbols_are_declared_exported_and_bound(lib):
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "evac.h")).read(), flags=re.S)
    for name in ("evac_transformer_workspace_bytes", "evac_transformer_minibatch_grad"):
        assert re.search(rf"\b{name}\s*\(", text) and name in _lib.SIGNATURES
        getattr(lib, name)
    decl = re.search(r"int evac_transformer_minibatch_grad\((.*?)\);", text, re.S).group(1)
    assert len(decl.split(",")) == len(lib.evac_transformer_minibatch_grad.argtypes) == 20
    assert lib.evac_transformer_workspace_bytes.restype is C.c_int64
    body = re.search(r"typedef struct evac_transformer_block_grads \{(.*?)\} evac_transformer_block_grads_t;", text, re.S).group(1)
    fields = [f for f, _ in _lib.EvacTransformerBlockGrads._fields_]
    assert re.findall(r"\*(\w+)", body) == fields == [f for f, _ in _lib.EvacTransformerBlock._fields_] == list(TC.BLOCK_NAMES)
    # ... which is _BLOCK_TENSORS' order: the module's names, the struct's abbreviations
    short = {"attention.Wq": "q", "attention.Wk": "k", "attention.Wv": "v", "attention.dense": "dense_", "ff[0]": "ff1_", "ff[3]": "ff2_",
             "norm1": "norm1_", "norm2": "norm2_"}
    as_fields = []
    for name in _BLOCK_TENSORS:
        mod, kind = name.rsplit(".", 1)
        s = short[mod]
        as_fields.append(("w" if kind == "weight" else "b") + s if len(s) == 1 else s + ("w" if kind == "weight" else "b"))
    assert as_fields == fields
    assert C.sizeof(_lib.EvacTransformerGrads) == 2 * 16 * 8
    assert lib.evac_version() == _lib.VERSION == 150
    assert os.path.join(build.CSRC, UNIT) in build.SOURCES


class Call(G.GradCall):
    """A call of evac_transformer_minibatch_grad whose every argument is acceptable, to be spoiled one argument at a time."""

    def __init__(self, D=36, dm=3, M=4, B=8, norm_adv=1, blocks=2):
        super().__init__(D, M, B, norm_adv)
        self.enc = _lib.EvacTransformer(dm, blocks, 3, 96, 0, 1e-5)
        self.enc_grads = _lib.EvacTransformerGrads()
        for b in range(2):
            self.enc.blocks[b] = _lib.EvacTransformerBlock(*[FAKE] * 16)
            self.enc_grads.blocks[b] = _lib.EvacTransformerBlockGrads(*[FAKE] * 16)

    def __call__(self, lib):
        return self.grad_call(lib.evac_transformer_minibatch_grad)


def test_every_refusal_comes_before_a_device_is_touched_with_its_code(lib):
    spoiled = []

    def add(why, code=BAD, **kw):
        c = Call(**kw)
        spoiled.append((why, code, c))
        return c
    G.rpo_refusals(add, "dm")
    # the encoder's: INVALID_ARGUMENT
    add("NULL encoder").null.add("enc")
    add("NULL encoder gradients").null.add("enc_grads")
    for b in range(2):
        for f in TC.BLOCK_NAMES:
            setattr(add(f"NULL encoder.blocks[{b}].{f}").enc.blocks[b], f, None)
            setattr(add(f"NULL encoder_grads.blocks[{b}].{f}").enc_grads.blocks[b], f, None)
    add("elem_dim 0").enc.elem_dim = 0
    add("elem_dim -1").enc.elem_dim = -1
    add("elem_dim 7", D=42, dm=7)
    add("elem_dim 5, which does not divide obs_dim", D=36, dm=5)
    add("obs_dim no multiple of elem_dim", D=37, dm=3)
    add("two tokens", D=12, dm=6)
    add("one token", D=6, dm=6)
    # ... UNSUPPORTED
    add("num_heads 2", UNSUPPORTED).enc.num_heads = 2
    add("num_heads 4", UNSUPPORTED).enc.num_heads = 4
    add("dim_feedforward 64", UNSUPPORTED).enc.dim_feedforward = 64
    add("num_blocks 0", UNSUPPORTED).enc.num_blocks = 0
    add("num_blocks 3", UNSUPPORTED).enc.num_blocks = 3
    add("ln_eps 1e-6", UNSUPPORTED).enc.ln_eps = 1e-6
    add("65 tokens (N = 63)", UNSUPPORTED, D=65 * 6, dm=6)
    add("66 tokens (N = 64)", UNSUPPORTED, D=66 * 6, dm=6)
    add("130 tokens of 3", UNSUPPORTED, D=390, dm=3)
    # sizes before pointers: an unsupported size with a NULL tensor is UNSUPPORTED; the linear network's refusals come first
    c = add("num_heads 2 and a NULL tensor", UNSUPPORTED)
    c.enc.num_heads, c.enc.blocks[0].wq = 2, None
    c = add("65 tokens and a NULL tensor", UNSUPPORTED, D=65 * 6, dm=6)
    c.enc.blocks[1].norm2_b = None
    c = add("65 tokens and a NULL gradient", UNSUPPORTED, D=65 * 6, dm=6)
    c.enc_grads.blocks[0].wk = None
    c = add("two tokens and a NULL tensor")
    c.enc.elem_dim, c.pol.obs_dim, c.enc.blocks[0].wq = 6, 12, None
    c = add("one block in use, a NULL gradient in it", blocks=1)
    c.enc_grads.blocks[0].bv = None
    c = add("num_heads 2 under a NULL stats", BAD)
    c.enc.num_heads, c.ptr["stats"] = 2, None
    assert len(spoiled) >= 130
    for why, code, c in spoiled:
        assert c(lib) == code, why
    assert BAD != UNSUPPORTED
    assert Call(M=1, norm_adv=0).cfg.norm_adv == 0   # (one sample without norm_adv is no refusal: not called, nothing to run it on)


def test_workspace_bytes(lib):
    f, g = lib.evac_transformer_workspace_bytes, lib.evac_rpo_workspace_bytes
    for D in (6, 36, 124, 372, 384, 396):
        prev = 0
        for M in (1, 2, 63, 64, 65, 1000, 4096, 16384, 16385, 20000, 100000, (1 << 31) - 1):
            n = f(D, M)
            assert n >= g(D, M) > 0 and n >= prev and n % 16 == 0, (D, M, n)
            # Y and dX (and the first block's output), the gathered columns and the index vector all fit
            assert n >= g(D, M) + M * (2 * D + 6) * 4 + M * 8
            prev = n
    for D, M in ((0, 64), (397, 64), (-1, 64), (36, 0), (36, -5), (36, 1 << 31)):
        assert f(D, M) == BAD and g(D, M) == BAD, (D, M)


NEW_KERNELS = ("k_tf_encode", "k_tf_dy", "k_tf_backward", "k_tf_finish")


def test_kernel_resources():
    """Seven kernels: the three of the linear gradient as the deep-sets unit instantiates them, and four of the encoder's.  None
    spills a vector register or uses scratch (measured: 0 and 0 for all four new kernels, pinned)."""
    kernels = kernel_resources(UNIT)
    names = [n.split("(")[0] for n in kernels]
    for stem in NEW_KERNELS + ("k_rpo_adv_stats<>", "k_rpo_grad<>", "k_rpo_finish<>"):
        assert sum(stem in n for n in names) == 1, (stem, names)
    assert len(kernels) == 7, names
    for name, k in kernels.items():
        assert k["private_segment_fixed_size"] == 0 and k["vgpr_spill_count"] == 0, (name, k)
    # the other units' kernels are as they were
    assert len(kernel_resources("evac_transformer_api.hip")) == 8
    assert len(kernel_resources("evac_deepsets_train_api.hip")) == 6


def test_static_lds_fits_a_cu():
    with tempfile.TemporaryDirectory() as tmp:
        out = os.path.join(tmp, "unit.s")
        flags = [f for f in build.FLAGS if f not in ("-fPIC", "-shared")]
        subprocess.run([build.hipcc_path()] + flags + ["-S", "--cuda-device-only", os.path.join(build.CSRC, UNIT), "-o", out],
                       check=True, capture_output=True)
        text = open(out).read()
    found = [int(v) for v in re.findall(r"\.group_segment_fixed_size:\s+(\d+)", text)]
    assert len(found) == 7 and max(found) <= 163840, found
    assert max(found) <= 65536                                       # (no kernel of the unit needs the limit raised)


CPU_CASES = [(10, 3, 64, 2, False, "strided", 1, 1, 0.01, 0.5), (5, 6, 100, 1, True, "repeat", 0, 0, 0.0, 0.0),
             (12, 2, 64, 2, False, "repeat", 1, 0, 0.0, 0.5)]


@pytest.mark.parametrize("N,ed,M,blocks,resid,mode,norm_adv,clip_vloss,ent,alpha", CPU_CASES)
def test_the_yardstick_agrees_with_the_trainers_autograd_path(N, ed, M, blocks, resid, mode, norm_adv, clip_vloss, ent, alpha):
    """The float32 yardstick (tests/trainer_ref.py's loss on `embedding`'s output, differentiated in two stages over chunks of
    rows) and autograd_minibatch_grad (the module itself, in one piece) are the same function: both within 4 x the yardstick's
    own float32-against-float64 error of float64."""
    from evacuation_amd import trainer
    from tests.test_gpu_trainer import stat_errors
    cfg = loss_cfg(norm_adv, clip_vloss, ent, alpha)
    net, batch, inds, z, g64, s64, t = TC.build_case(N, ed, M, blocks, resid, mode, cfg, seed=N + M, device="cpu")
    g32, s32, _ = TC.minibatch_grad(net, batch, inds, cfg, z, rows=48)         # (more than one chunk)
    stats = torch.zeros(8)
    trainer.autograd_minibatch_grad(TC.fake_trainer(net, cfg), batch, inds, z, 0, stats)
    ga = [p.grad.clone() for p in TC.all_tensors(net)]
    assert len(ga) == len(g64) == 13 + 16 * blocks == len(TC.names(blocks))
    TC.assert_key_biases_are_zero(g64, blocks)
    e32, ea_ = TC.tensor_errors(g32, g64, blocks), TC.tensor_errors(ga, g64, blocks)
    bound = 4 * max(e32) + 1e-7
    for name, e in zip(TC.names(blocks), ea_):
        assert e <= bound, (name, e, bound)
    sbound = 4 * max(stat_errors(s32, s64)) + 1e-7
    for name, e in zip(TC.R.STATS, stat_errors(stats, s64)):
        assert e <= sbound, (name, e, sbound)
    others = [g for i, g in enumerate(g64) if i >= 13 and i not in TC.key_biases(blocks)]
    assert all(float(g.abs().max()) > 0 for g in others)                       # the encoder's gradients are there


def test_build_case_conditions_hold_on_the_largest_gpu_case():
    cfg = loss_cfg(1, 1, 0.0, 0.5)
    net, batch, inds, z, g64, s64, t = TC.build_case(60, 6, 2048, 2, True, "repeat", cfg, seed=7, device="cpu", cache=False)
    assert batch["b_obs"].shape == (2048, 372) and len(g64) == 45
    net64 = TC.twin_of(net, torch.float64)
    pre_min, var_min, _ = TC.internals(net64, batch["b_obs"].double())
    assert float(pre_min.min()) >= TC.RELU_MARGIN and float(var_min.min()) >= TC.VARIANCE_FLOOR
    assert t.pre_min == float(pre_min.min()) and t.var_min == float(var_min.min())


def test_what_stays_as_it_was_for_such_a_network():
    from evacuation_amd import trainer
    net = TransformerActorCritic(36, 10)
    cfg = trainer.RPOTrainingConfig(num_envs=4, num_steps=8, num_minibatches=2)
    env = SimpleNamespace(num_envs=4)
    tr = trainer.RPOTrainer(env, net, cfg)
    assert tr.grad_fn is trainer.autograd_minibatch_grad and callable(trainer.transformer_kernel_grad)
    opted = trainer.RPOTrainer(env, net, cfg, grad_fn=trainer.transformer_kernel_grad)
    assert opted.grad_fn is trainer.transformer_kernel_grad and isinstance(opted.optimizer, torch.optim.Adam)
    with pytest.raises(ValueError, match="`embedding`"):
        trainer.RPOTrainer(env, net, cfg, optimizer="device", grad_fn=trainer.transformer_kernel_grad)
    assert all(trainer.transformer_kernel_grad is not fn for fn, _ in trainer._STEP_OF + trainer._UPDATE_OF)
    assert len(trainer._STEP_OF) == len(trainer._UPDATE_OF) == 2
    batch = {"b_obs": torch.zeros(8, 36)}
    inds = torch.zeros(4, dtype=torch.int64)
    with pytest.raises(ValueError, match="no attention encoder"):
        trainer.transformer_minibatch_grad(LinearActorCritic(36), batch, inds, loss_cfg())
    with pytest.raises(ValueError, match="`embedding` has dropout p = 0.1"):
        trainer.transformer_minibatch_grad(TransformerActorCritic(36, 10, dropout=0.1), batch, inds, loss_cfg())
