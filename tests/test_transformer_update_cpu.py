"""CPU tests of the transformer leader's optimiser step and whole update (include/evac.h: evac_transformer_adam_step,
evac_transformer_minibatch_step, evac_transformer_update): the symbols, every refusal with no device present (no pointer is ever
followed: they are made-up addresses) with the code of each cause, the compiled kernels of the new translation unit, and the
Python entries' argument errors."""
import ctypes as C
import os
import re
from types import SimpleNamespace

import pytest
import torch

from evacuation_amd import _lib, build
from evacuation_amd.policy import DeepSetsActorCritic, LinearActorCritic, TransformerActorCritic
from tests import encoder_grad_cases as G
from tests import transformer_grad_cases as TC
from tests.encoder_grad_cases import BATCH, FAKE
from tests.kernel_meta import kernel_resources

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BAD, UNSUPPORTED = _lib.ERR_INVALID_ARGUMENT, _lib.ERR_UNSUPPORTED
ENTRIES = ("evac_transformer_adam_step", "evac_transformer_minibatch_step", "evac_transformer_update")
UNIT = "evac_transformer_update_api.hip"


@pytest.fixture(scope="module")
def lib():
    build.build_library()
    return _lib.load()


def test_symbols_are_declared_exported_and_bound(lib):
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "evac.h")).read(), flags=re.S)
    counts = {}
    for name in ENTRIES + ("evac_transformer_minibatch_grad", "evac_deepsets_adam_step", "evac_rpo_update", "evac_deepsets_update"):
        decl = re.search(rf"int {name}\((.*?)\);", text, re.S)
        assert decl and name in _lib.SIGNATURES, name
        fn = getattr(lib, name)
        counts[name] = len(decl.group(1).split(","))
        assert len(fn.argtypes) == counts[name] and fn.restype is C.c_int, name
    assert counts["evac_transformer_minibatch_step"] == counts["evac_transformer_minibatch_grad"] + 4 == 24
    assert counts["evac_transformer_update"] == counts["evac_rpo_update"] + 3 == counts["evac_deepsets_update"]
    assert counts["evac_transformer_adam_step"] == counts["evac_deepsets_adam_step"] + 1 == 11       # (num_blocks)
    sig, grads, enc_grads = _lib.SIGNATURES, C.POINTER(_lib.EvacMlpPolicyGrads), C.POINTER(_lib.EvacTransformerGrads)
    assert sig["evac_transformer_minibatch_step"][1] == sig["evac_transformer_minibatch_grad"][1] + [
        grads, enc_grads, C.POINTER(_lib.EvacTransformerAdamState), C.POINTER(_lib.EvacAdamConfig)]
    swap = {C.POINTER(_lib.EvacDeepSets): C.POINTER(_lib.EvacTransformer), C.POINTER(_lib.EvacDeepSetsGrads): enc_grads,
            C.POINTER(_lib.EvacDeepSetsAdamState): C.POINTER(_lib.EvacTransformerAdamState)}
    assert sig["evac_transformer_update"][1] == [swap.get(t, t) for t in sig["evac_deepsets_update"][1]]
    body = re.search(r"typedef struct evac_transformer_adam_state \{(.*?)\} evac_transformer_adam_state_t;", text, re.S).group(1)
    assert re.findall(r"(\w+)[,;]", body) == [f for f, _ in _lib.EvacTransformerAdamState._fields_] == \
        ["header", "exp_avg", "exp_avg_sq", "enc_exp_avg", "enc_exp_avg_sq"]
    assert C.sizeof(_lib.EvacTransformerAdamState) == 8 + 2 * 13 * 8 + 2 * 32 * 8
    for f in ("header", "exp_avg", "exp_avg_sq"):
        assert getattr(_lib.EvacTransformerAdamState, f).offset == getattr(_lib.EvacAdamState, f).offset, f
    assert os.path.join(build.CSRC, UNIT) in build.SOURCES


# ------------------------------------------------------------------------------------------------ refusals
def _block(cls):
    return cls(*[FAKE] * 16)


class Call(G.GradCall):
    """A call of one of the three entries whose every argument is acceptable, to be spoiled one argument at a time."""

    def __init__(self, entry, D=36, dm=3, M=4, B=8, norm_adv=1, epochs=2, blocks=2):
        super().__init__(D, M, B, norm_adv)
        self.entry = entry
        self.enc = _lib.EvacTransformer(dm, blocks, 3, 96, 0, 1e-5)
        self.enc_grads, self.enc_params = _lib.EvacTransformerGrads(), _lib.EvacTransformerGrads()
        self.state = _lib.EvacTransformerAdamState(FAKE, _lib.EvacMlpPolicyGrads(*[FAKE] * 13), _lib.EvacMlpPolicyGrads(*[FAKE] * 13),
                                                   _lib.EvacTransformerGrads(), _lib.EvacTransformerGrads())
        for b in range(2):
            self.enc.blocks[b] = _block(_lib.EvacTransformerBlock)
            for st in (self.enc_grads, self.enc_params, self.state.enc_exp_avg, self.state.enc_exp_avg_sq):
                st.blocks[b] = _block(_lib.EvacTransformerBlockGrads)
        self.params = _lib.EvacMlpPolicyGrads(*[FAKE] * 13)
        self.adam = _lib.EvacAdamConfig(3e-4, 0.9, 0.999, 1e-5, 0.5)
        self.D, self.dm, self.epochs, self.blocks = D, dm, epochs, blocks
        self.ptr["sumsq"] = FAKE

    def encoder_structs(self):
        """name -> struct, of the four that hold the optimiser's 16 pointers per block."""
        return {"enc_params": self.enc_params, "enc_grads": self.enc_grads, "enc_exp_avg": self.state.enc_exp_avg,
                "enc_exp_avg_sq": self.state.enc_exp_avg_sq}

    def __call__(self, lib):
        ref, p = self.ref, self.ptr
        batch = [self.B] + [p[k] for k in BATCH]
        if self.entry == "evac_transformer_adam_step":
            return lib.evac_transformer_adam_step(ref("params"), ref("enc_params"), ref("grads"), ref("enc_grads"), ref("state"),
                                                  ref("adam"), self.D, self.dm, self.blocks, p["sumsq"], None)
        if self.entry == "evac_transformer_minibatch_step":
            return self.grad_call(lib.evac_transformer_minibatch_step, ref("params"), ref("enc_params"), ref("state"), ref("adam"))
        return lib.evac_transformer_update(ref("pol"), ref("enc"), ref("params"), ref("enc_params"), ref("grads"), ref("enc_grads"),
                                           ref("cfg"), ref("adam"), ref("state"), *batch, self.M, self.epochs, p["mb_inds"], None, 1, 2, 1,
                                           0.01, p["stats"], p["workspace"], None)


BAD_ADAM = [("lr", float("nan")), ("lr", float("inf")), ("lr", -float("inf")), ("beta1", -0.1), ("beta1", 1.0), ("beta1", float("nan")),
            ("beta2", -1e-9), ("beta2", 1.0), ("beta2", 1.5), ("eps", 0.0), ("eps", -1e-5), ("eps", float("nan")),
            ("max_grad_norm", 0.0), ("max_grad_norm", -0.5), ("max_grad_norm", float("nan"))]
MLP_FIELDS = [f for f, _ in _lib.EvacMlpPolicyGrads._fields_]


def spoiled_calls(entry):
    spoiled = []
    step_only = entry == "evac_transformer_adam_step"

    def add(why, code=BAD, **kw):
        c = Call(entry, **kw)
        spoiled.append((why, code, c))
        return c

    def set_blocks(c, n):
        """``n`` blocks in use, in the step's argument and in the encoder's struct (which the other two entries read)."""
        c.blocks = c.enc.num_blocks = n
        return c
    # what evac_adam_step refuses, and the encoder's part of the optimiser
    for s in ("params", "enc_params", "grads", "enc_grads", "state", "adam"):
        add(f"NULL {s}").null.add(s)
    for f in MLP_FIELDS:
        setattr(add(f"NULL params.{f}").params, f, None)
        setattr(add(f"NULL grads.{f}").grads, f, None)
        setattr(add(f"NULL exp_avg.{f}").state.exp_avg, f, None)
        setattr(add(f"NULL exp_avg_sq.{f}").state.exp_avg_sq, f, None)
    for which in ("enc_params", "enc_grads", "enc_exp_avg", "enc_exp_avg_sq"):
        for b in range(2):
            for f in TC.BLOCK_NAMES:
                setattr(add(f"NULL {which}.blocks[{b}].{f}").encoder_structs()[which].blocks[b], f, None)
        # one block in use: a NULL tensor in it is refused ...
        c = set_blocks(add(f"one block in use, NULL {which}.blocks[0].ff1_w"), 1)
        c.encoder_structs()[which].blocks[0].ff1_w = None
    add("NULL header").state.header = None
    add("misaligned header").state.header = FAKE + 4
    for f, v in BAD_ADAM:
        setattr(add(f"{f} = {v}").adam, f, v)
    add("obs_dim 0", D=0)
    add("obs_dim 397", D=397, dm=1)
    add("elem_dim 0", dm=0)
    add("elem_dim -1", dm=-1)
    add("elem_dim 5, which does not divide obs_dim", D=36, dm=5)
    add("elem_dim 7", D=42, dm=7)
    add("obs_dim no multiple of elem_dim", D=37, dm=3)
    add("two tokens", D=12, dm=6)
    add("one token", D=6, dm=6)
    # ... UNSUPPORTED: the sizes, looked at before the encoder's pointers and behind the linear network's refusals
    set_blocks(add("num_blocks 0", UNSUPPORTED), 0)
    set_blocks(add("num_blocks 3", UNSUPPORTED), 3)
    set_blocks(add("num_blocks -1", UNSUPPORTED), -1)
    add("65 tokens (N = 63)", UNSUPPORTED, D=65 * 6, dm=6)
    add("66 tokens (N = 64)", UNSUPPORTED, D=66 * 6, dm=6)
    add("130 tokens of 3", UNSUPPORTED, D=390, dm=3)
    add("65 tokens and a NULL moment", UNSUPPORTED, D=65 * 6, dm=6).state.enc_exp_avg.blocks[1].norm2_b = None
    add("65 tokens and a NULL parameter", UNSUPPORTED, D=65 * 6, dm=6).enc_params.blocks[0].wq = None
    set_blocks(add("num_blocks 3 and a NULL parameter", UNSUPPORTED), 3).enc_params.blocks[0].wq = None
    add("two tokens and a NULL parameter", D=12, dm=6).enc_params.blocks[0].wq = None
    if step_only:                                                            # (the other two look at the encoder's sizes first)
        set_blocks(add("num_blocks 3 under a NULL exp_avg.actor_w1"), 3).state.exp_avg.actor_w1 = None
        set_blocks(add("num_blocks 3 under lr = nan"), 3).adam.lr = float("nan")
        add("NULL grad_sumsq").ptr["sumsq"] = None
        add("65 tokens under a NULL grad_sumsq", UNSUPPORTED, D=65 * 6, dm=6).ptr["sumsq"] = None
        return spoiled
    # everything evac_transformer_minibatch_grad refuses (rpo_prepare's, then the encoder's)
    G.rpo_refusals(add, "dm", own_grads=False)
    add("NULL enc").null.add("enc")
    for b in range(2):
        for f in TC.BLOCK_NAMES:
            setattr(add(f"NULL encoder.blocks[{b}].{f}").enc.blocks[b], f, None)
    add("num_heads 2", UNSUPPORTED).enc.num_heads = 2
    add("dim_feedforward 64", UNSUPPORTED).enc.dim_feedforward = 64
    add("ln_eps 1e-6", UNSUPPORTED).enc.ln_eps = 1e-6
    c = add("num_heads 2 and a NULL moment", UNSUPPORTED)
    c.enc.num_heads, c.state.enc_exp_avg_sq.blocks[0].wq = 2, None
    c = add("num_heads 2 under a NULL stats")
    c.enc.num_heads, c.ptr["stats"] = 2, None
    add("the encoder's elem_dim differs: 0").enc.elem_dim = 0
    if entry == "evac_transformer_update":
        add("n_epochs 0", epochs=0)
        add("n_epochs -1", epochs=-1)
        c = add("n_epochs 0 and num_heads 2", epochs=0)
        c.enc.num_heads = 2
    return spoiled


@pytest.mark.parametrize("entry,least", [("evac_transformer_adam_step", 220), ("evac_transformer_minibatch_step", 220 + 30 + 32),
                                         ("evac_transformer_update", 220 + 30 + 32 + 2)])
def test_every_refusal_comes_before_a_device_is_touched_with_its_code(lib, entry, least):
    """One spoiled argument at a time, nothing ever followed: the 13 tensors' 58 and the encoder's 4 x 32 NULL pointers, the Adam
    configuration's 15, the header's 2, the sizes; for the step and the update everything the gradient refuses on top."""
    spoiled = spoiled_calls(entry)
    assert len(spoiled) >= least, len(spoiled)
    assert len({why for why, _, _ in spoiled}) == len(spoiled)
    assert BAD != UNSUPPORTED and BAD < 0 and UNSUPPORTED < 0
    for why, code, c in spoiled:
        assert c(lib) == code, (entry, why)
    # (That a block NOT in use may be NULL everywhere has no code of its own to show here -- nothing is checked behind the blocks'
    # pointers but the step's grad_sumsq, with the same code -- so tests/test_gpu_transformer_update.py shows it: its one-block
    # cases run with blocks[1] NULL in the parameters, the gradients and both moments.)


# ------------------------------------------------------------------------------------------------ the compiled kernels
GATED = "<evac::AdamHeader const*>"
TWIN_FIELDS = ("vgpr_count", "vgpr_spill_count", "sgpr_spill_count", "private_segment_fixed_size")
GRAD_STEMS = ("k_tf_encode", "k_tf_dy", "k_tf_backward", "k_tf_finish", "k_rpo_adv_stats", "k_rpo_grad", "k_rpo_finish")


def stems(unit):
    by_stem = {}
    for name, k in kernel_resources(unit).items():
        stem = re.sub(r"^void ", "", name.split("(")[0]).replace("evac::", "", 1)
        assert stem not in by_stem, name
        by_stem[stem] = k
    return by_stem


def test_kernels_of_the_new_unit():
    """evac_transformer_update_api.hip holds k_adam_tf once and the seven gradient kernels twice: plain (the step's) and gated by
    the optimiser's header (the update's): 15 kernels, none with scratch or a spilled vector register; a gated instantiation has
    its plain twin's figures.  k_adam_tf (measured): 44 VGPRs, 42 SGPRs, 0 spilled SGPRs, 0 spilled VGPRs, no scratch -- the
    45-tensor argument struct is read from the kernel-argument segment where it lies."""
    by_stem = stems(UNIT)
    grads = [s + t for s in GRAD_STEMS for t in ("<>", GATED)]
    assert sorted(by_stem) == sorted(["k_adam_tf"] + grads) and len(by_stem) == 15, sorted(by_stem)
    adam = by_stem["k_adam_tf"]
    print("\nk_adam_tf:", adam)
    assert adam["private_segment_fixed_size"] == 0 and adam["vgpr_spill_count"] == 0, adam
    assert adam["sgpr_spill_count"] == 0, adam                               # (measured: 0)
    assert adam["vgpr_count"] <= 128, adam
    for stem in grads:
        k = by_stem[stem]
        assert k["private_segment_fixed_size"] == 0 and k["vgpr_spill_count"] == 0, (stem, k)
        if stem.endswith(GATED):
            plain = by_stem[stem.replace(GATED, "<>")]
            print(stem, k, "| plain:", plain)
            for f in TWIN_FIELDS:
                assert k[f] == plain[f], (stem, f, k, plain)
    # the gradient unit's own kernels, under their names: the plain instantiations, with the same figures
    own = stems("evac_transformer_train_api.hip")
    assert sorted(own) == sorted(s for s in grads if s.endswith("<>"))
    for stem, k in own.items():
        assert k == by_stem[stem], (stem, k, by_stem[stem])
    # the other units' kernels are as they were
    assert len(kernel_resources("evac_transformer_api.hip")) == 8
    assert len(kernel_resources("evac_deepsets_train_api.hip")) == 6
    assert len(kernel_resources("evac_deepsets_update_api.hip")) == 13


# ------------------------------------------------------------------------------------------------ Python argument errors
def test_python_argument_errors_without_a_device():
    from evacuation_amd import trainer
    tf, linear, deep = TransformerActorCritic(36, 10), LinearActorCritic(36), DeepSetsActorCritic(36, 10)
    for net in (linear, deep):
        with pytest.raises(ValueError, match="no attention encoder"):
            trainer.TransformerAdam(net)
    with pytest.raises(ValueError, match="`embedding` has dropout p = 0.1"):
        trainer.TransformerAdam(TransformerActorCritic(36, 10, dropout=0.1))
    with pytest.raises(ValueError, match="contiguous float32 device tensors"):   # (its own refusals passed: it needs a device)
        trainer.TransformerAdam(tf)
    assert issubclass(trainer.TransformerAdam, trainer.DeviceAdam)
    # DeviceAdam and optimizer="device" keep refusing such a network
    with pytest.raises(ValueError, match="`embedding`"):
        trainer.DeviceAdam(tf)
    cfg = trainer.RPOTrainingConfig(num_envs=4, num_steps=8, num_minibatches=2)
    env = SimpleNamespace(num_envs=4)
    for grad_fn in (None, trainer.transformer_kernel_grad, trainer.autograd_minibatch_grad):
        with pytest.raises(ValueError, match="`embedding`"):
            trainer.RPOTrainer(env, tf, cfg, optimizer="device", grad_fn=grad_fn)
    # the third optimiser kind: for a network with an attention encoder and an explicit grad_fn alone
    for net in (linear, deep):
        with pytest.raises(ValueError, match="device_transformer.*no attention encoder"):
            trainer.RPOTrainer(env, net, cfg, optimizer="device_transformer", grad_fn=trainer.transformer_kernel_grad)
    with pytest.raises(ValueError, match="device_transformer.*explicit grad_fn"):
        trainer.RPOTrainer(env, tf, cfg, optimizer="device_transformer")
    with pytest.raises(ValueError, match="dropout p = 0.1"):
        trainer.RPOTrainer(env, TransformerActorCritic(36, 10, dropout=0.1), cfg, optimizer="device_transformer",
                           grad_fn=trainer.transformer_kernel_grad)
    with pytest.raises(ValueError, match="nonsense"):
        trainer.RPOTrainer(env, tf, cfg, optimizer="nonsense")
    # the entries' own optimiser check
    batch = {"b_obs": torch.zeros(8, 36)}
    inds, perms = torch.arange(4), torch.arange(8)[None]
    opt = object.__new__(trainer.TransformerAdam)                             # (a TransformerAdam needs a device: one of another network)
    opt.net = TransformerActorCritic(36, 10)
    for fn, arg in ((trainer.transformer_minibatch_step, inds), (trainer.transformer_update, perms)):
        for net in (linear, deep):
            with pytest.raises(ValueError, match="no attention encoder"):
                fn(net, batch, arg, cfg, opt)
        with pytest.raises(ValueError, match="made for another network"):
            fn(tf, batch, arg, cfg, opt)
        with pytest.raises(TypeError, match="expected a TransformerAdam"):
            fn(tf, batch, arg, cfg, SimpleNamespace(net=tf))
        with pytest.raises(ValueError, match="dropout p = 0.1"):
            fn(TransformerActorCritic(36, 10, dropout=0.1), batch, arg, cfg, opt)
    # ... and the other networks' entries keep refusing such a network, whatever the optimiser
    opt.net = tf
    for fn, arg in ((trainer.rpo_minibatch_step, inds), (trainer.rpo_update, perms), (trainer.deepsets_minibatch_step, inds),
                    (trainer.deepsets_update, perms)):
        with pytest.raises(ValueError, match="`embedding`"):
            fn(tf, batch, arg, cfg, opt)
    # the one-call tables: the two rows they had, and a pair of their own for the third kind
    assert len(trainer._STEP_OF) == len(trainer._UPDATE_OF) == 2
    assert set(trainer._ONE_CALL_TABLES) == {"device", "device_transformer"}
    assert trainer._ONE_CALL_TABLES["device"] == (trainer._STEP_OF, trainer._UPDATE_OF)
    assert trainer._ONE_CALL_TABLES["device_transformer"] == (((trainer.transformer_kernel_grad, trainer.transformer_minibatch_step),),
                                                              ((trainer.transformer_kernel_grad, trainer.transformer_update),))
    for what in ("adam_step", "minibatch_step", "update"):
        from evacuation_amd.policy import encoder_kind
        assert trainer._entry_name(encoder_kind(tf), what) == f"evac_transformer_{what}" in _lib.SIGNATURES
