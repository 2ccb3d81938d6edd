"""CPU tests of the update of a population of transformer leaders (include/evac.h: evac_transformer_population_workspace_bytes,
evac_transformer_update_population; evacuation_amd.population.TransformerPopulationAdam, transformer_update_population,
PopulationTrainer(optimizer="device_transformer")): the symbols, the workspace's size, every refusal with no device present (no
pointer is ever followed: they are made-up addresses), the build's sources, the compiled kernels of the new translation unit and
the Python faces on the CPU."""
import ctypes as C
import dataclasses
import os
import re
from types import SimpleNamespace

import pytest
import torch

from evacuation_amd import _lib, build
from tests import kernel_meta

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BAD, UNSUPPORTED = _lib.ERR_INVALID_ARGUMENT, _lib.ERR_UNSUPPORTED
FAKE = 0x1000                                    # 16-byte aligned, never followed
UNIT = "evac_transformer_population_update_api.hip"
BLOCK_FIELDS = [f for f, _ in _lib.EvacTransformerBlockStrides._fields_]


@pytest.fixture(scope="module")
def lib():
    build.build_library()
    return _lib.load()


def test_symbols_are_declared_exported_and_bound(lib):
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "evac.h")).read(), flags=re.S)
    counts = {}
    for name in ("evac_transformer_update_population", "evac_deepsets_update_population"):
        decl = re.search(rf"int {name}\((.*?)\);", text, re.S)
        assert decl and name in _lib.SIGNATURES, name
        fn = getattr(lib, name)
        counts[name] = len(decl.group(1).split(","))
        assert len(fn.argtypes) == counts[name] and fn.restype is C.c_int, name
    assert counts["evac_transformer_update_population"] == counts["evac_deepsets_update_population"] == 36
    params = re.search(r"int evac_transformer_update_population\((.*?)\);", text, re.S).group(1).split(",")
    assert "evac_transformer_t" in params[2] and "evac_transformer_grads_t" in params[4] and "evac_transformer_grads_t" in params[6]
    assert all("evac_transformer_strides_t" in params[i] for i in (8, 10, 12)) and "evac_transformer_adam_state_t" in params[16]
    assert re.search(r"int64_t evac_transformer_population_workspace_bytes\(int32_t \w+, int64_t \w+, int32_t \w+\);", text)
    assert "evac_transformer_population_workspace_bytes" in _lib.SIGNATURES
    sizer = lib.evac_transformer_population_workspace_bytes
    assert sizer.restype is C.c_int64 and len(sizer.argtypes) == 3
    assert lib.evac_version() == _lib.VERSION == 150
    # the comment above the strides' struct no longer says that the update does not exist
    above = open(os.path.join(ROOT, "include", "evac.h")).read().split("typedef struct evac_transformer_block_strides")[0][-1500:]
    assert "does not exist: each learner" not in above and "evac_transformer_update_population" in above


def test_the_unit_is_built_before_the_capture_unit():
    unit = os.path.join(build.CSRC, UNIT)
    assert unit in build.SOURCES and unit in build.DEPENDS
    assert os.path.basename(build.SOURCES[-1]) == "evac_capture_api.hip"
    for header in ("evac_transformer_population_train.h", "evac_transformer_adam_host.h", "evac_transformer_adam_args.h"):
        assert os.path.join(build.CSRC, header) in build.DEPENDS, header
    # the moved host code: one definition, in the shared header
    lone = open(os.path.join(build.CSRC, "evac_transformer_update_api.hip")).read()
    shared = open(os.path.join(build.CSRC, "evac_transformer_adam_host.h")).read()
    assert "int tf_adam_prepare(" not in lone and "inline int tf_adam_prepare(" in shared and "tf_adam_launch(" in shared


# ------------------------------------------------------------------------------------------------ the workspace's size
def round256(n):
    return (n + 255) // 256 * 256


def test_workspace_bytes(lib):
    pop, one = lib.evac_transformer_population_workspace_bytes, lib.evac_transformer_workspace_bytes
    for D, M in ((9, 8), (36, 70), (72, 3), (372, 192), (384, 1024)):
        lone = one(D, M)
        assert lone > 0
        for S in (1, 2, 3, 8, 64):
            rows = S * M
            common = round256(rows * D * 4) + round256(rows * 2 * 4) + 4 * round256(rows * 4) + round256(rows * 8)
            assert pop(D, M, S) == S * round256(lone) + common, (D, M, S)
            assert round256(lone) % 256 == 0 and (pop(D, M, S) - common) // S % 256 == 0      # every slice: whole 256-byte parts
    for bad in ((0, 64, 2), (397, 64, 2), (6, 0, 2), (6, -1, 2)):       # whatever the lone sizer refuses
        assert one(*bad[:2]) == BAD and pop(*bad) == BAD, bad
    for S in (0, -1, 65):
        assert pop(36, 64, S) == BAD, S


# ------------------------------------------------------------------------------------------------ refusals
def block_sizes(dm):
    return [3 * dm * dm, 3 * dm, 3 * dm * dm, 3 * dm, 3 * dm * dm, 3 * dm, 3 * dm * dm, dm, 96 * dm, 96, 96 * dm, dm, dm, dm, dm, dm]


def mlp_sizes(D):
    return [64 * D, 64, 64 * 64, 64, 128, 2, 2, 64 * D, 64, 64 * 64, 64, 64, 1]


def enc_strides(dm, blocks):
    st = _lib.EvacTransformerStrides()
    for b in range(blocks):
        st.blocks[b] = _lib.EvacTransformerBlockStrides(*block_sizes(dm))
    return st


def enc_grads(blocks):
    st = _lib.EvacTransformerGrads()
    for b in range(blocks):
        st.blocks[b] = _lib.EvacTransformerBlockGrads(*[FAKE] * 16)
    return st


class Update:
    """A call of evac_transformer_update_population whose every argument is acceptable, to be spoiled one argument at a time.
    The blocks beyond ``blocks`` hold NULL pointers and zero strides in every struct."""

    def __init__(self, S=2, D=36, dm=3, blocks=2, M=4, B_l=8, norm_adv=1, epochs=2):
        self.S, self.D, self.dm, self.M, self.B_l, self.epochs = S, D, dm, M, B_l, epochs
        self.pol = _lib.EvacMlpPolicy(D, 64, *[FAKE] * 13)
        self.enc = _lib.EvacTransformer(dm, blocks, 3, 96, 0, 1e-5)
        for b in range(blocks):
            self.enc.blocks[b] = _lib.EvacTransformerBlock(*[FAKE] * 16)
        self.params, self.grads = _lib.EvacMlpPolicyGrads(*[FAKE] * 13), _lib.EvacMlpPolicyGrads(*[FAKE] * 13)
        self.enc_params, self.enc_grads = enc_grads(blocks), enc_grads(blocks)
        self.strides = [_lib.EvacMlpPolicyStrides(*mlp_sizes(D)) for _ in range(3)]
        self.enc_strides = [enc_strides(dm, blocks) for _ in range(3)]
        self.header_stride = 64
        self.cfg = _lib.EvacRpoLossConfig(0.2, 0.0, 0.5, 0.5, norm_adv, 1)
        self.adam = _lib.EvacAdamConfig(3e-4, 0.9, 0.999, 1e-5, 0.5)
        self.state = _lib.EvacTransformerAdamState(FAKE, _lib.EvacMlpPolicyGrads(*[FAKE] * 13), _lib.EvacMlpPolicyGrads(*[FAKE] * 13),
                                                   enc_grads(blocks), enc_grads(blocks))
        self.null = set()                        # names of struct arguments passed as NULL
        self.seeds = self.counters = True
        self.workspace = FAKE
        self.batch = S * B_l

    def ref(self, name, obj):
        return None if name in self.null else C.byref(obj)

    def __call__(self, lib):
        u64 = (C.c_uint64 * max(self.S, 1))()
        r = self.ref
        return lib.evac_transformer_update_population(
            self.S, r("pol", self.pol), r("enc", self.enc), r("params", self.params), r("enc_params", self.enc_params),
            r("grads", self.grads), r("enc_grads", self.enc_grads), r("param_strides", self.strides[0]),
            r("enc_param_strides", self.enc_strides[0]), r("grad_strides", self.strides[1]), r("enc_grad_strides", self.enc_strides[1]),
            r("moment_strides", self.strides[2]), r("enc_moment_strides", self.enc_strides[2]), self.header_stride, r("cfg", self.cfg),
            r("adam", self.adam), r("state", self.state), self.batch, *[FAKE] * 6, self.B_l, self.M, self.epochs, FAKE, None,
            u64 if self.seeds else None, u64 if self.counters else None, 1, 0.01, FAKE, self.workspace, None)


def test_update_refusals_without_a_device(lib):
    """Every refusal is decided on the host: the pointers are made up, and a call that got past the checks would follow them.  So
    what the checks ACCEPT is shown here only up to the next check -- the optimiser's tensors, which come last and refuse a NULL
    moment: the acceptance itself (``blocks[1]`` strides of -5 in a one-block net) runs in
    tests/test_gpu_transformer_population_update.py."""
    def refused(call, why, code=BAD):
        assert call(lib) == code, why

    for S in (0, 65):
        refused(Update(S=S), f"n_learners {S}")
    for name in ("param_strides", "enc_param_strides", "grad_strides", "enc_grad_strides", "moment_strides", "enc_moment_strides",
                 "pol", "enc", "params", "enc_params", "grads", "enc_grads", "cfg", "adam", "state"):
        call = Update()
        call.null.add(name)
        refused(call, f"NULL {name}")
    for which in range(3):                       # parameters, gradients, moments
        for b in range(2):                       # two learners, both blocks in use
            for field, least in zip(BLOCK_FIELDS, block_sizes(3)):
                for value in (least - 1, 0):
                    call = Update()
                    setattr(call.enc_strides[which].blocks[b], field, value)
                    refused(call, f"encoder stride {which}.blocks[{b}].{field} = {value} with S = 2")
        call = Update()
        call.strides[which].actor_w1 = 64 * 36 - 1
        refused(call, f"policy stride {which} below its tensor")
    for which, sets in enumerate(("enc", "enc_params", "enc_grads")):   # a NULL tensor of a block in use
        call = Update()
        getattr(call, sets).blocks[1].ff2_w = None
        refused(call, f"NULL {sets}.blocks[1].ff2_w")
    for moments in ("enc_exp_avg", "enc_exp_avg_sq"):
        call = Update()
        getattr(call.state, moments).blocks[0].norm2_b = None
        refused(call, f"NULL state.{moments}.blocks[0].norm2_b")
    for stride in (56, 68):
        call = Update()
        call.header_stride = stride
        refused(call, f"header stride {stride}")
    call = Update()
    call.workspace = FAKE + 8
    refused(call, "a misaligned workspace")
    refused(Update(epochs=0), "n_epochs 0")
    refused(Update(B_l=0), "learner_batch_size 0")
    refused(Update(M=1), "one sample with norm_adv")
    refused(Update(dm=5, D=36), "D not a multiple of elem_dim")
    refused(Update(dm=3, D=6), "fewer than 3 tokens")
    refused(Update(dm=7, D=42), "elem_dim 7")
    refused(Update(dm=3, D=3 * 65), "65 tokens", UNSUPPORTED)
    call = Update()
    call.enc.num_blocks = 3
    refused(call, "num_blocks 3", UNSUPPORTED)
    for field, value in (("num_heads", 4), ("dim_feedforward", 64), ("ln_eps", 1e-6)):
        call = Update()
        setattr(call.enc, field, value)
        refused(call, f"{field} = {value}", UNSUPPORTED)
    for flag in ("seeds", "counters"):
        call = Update()
        setattr(call, flag, False)
        refused(call, f"NULL {flag}")
    # the order, by two double faults: the gradient's checks of the encoder come before the NULL state, and before the
    # population's own (the learners' number) and the encoder strides'
    call = Update()
    call.enc.num_heads = 4
    call.null.add("state")
    refused(call, "num_heads 4 and a NULL state: the encoder first", UNSUPPORTED)
    call = Update(S=0, dm=3, D=3 * 65)
    call.batch = 16                              # (the common batch itself is acceptable)
    call.enc_strides[0].blocks[0].wq = 0
    refused(call, "65 tokens, no learners and a zero stride: the encoder first", UNSUPPORTED)
    # a block NOT in use is never looked at: a one-block net whose blocks[1] holds NULL pointers everywhere and strides below
    # every tensor (and negative ones) gets to the last check, the optimiser's tensors, which refuses a NULL moment
    call = Update(blocks=1)
    for which in range(3):
        for field, least in zip(BLOCK_FIELDS, block_sizes(3)):
            setattr(call.enc_strides[which].blocks[1], field, -5 if which == 0 else least - 1)
    call.state.enc_exp_avg_sq.blocks[0].norm2_b = None
    refused(call, "one block with blocks[1] strides below their tensors, up to the optimiser's NULL moment")
    # S = 1: the strides are not held against the tensors (nobody is s x stride further)
    call = Update(S=1)
    for which in range(3):
        for b in range(2):
            for field in BLOCK_FIELDS:
                setattr(call.enc_strides[which].blocks[b], field, 0)
    call.header_stride = 0
    call.state.enc_exp_avg_sq.blocks[1].norm2_b = None
    refused(call, "S = 1 with zero strides, up to the optimiser's NULL moment")
    call = Update(S=1)
    call.null.add("enc_moment_strides")          # a NULL strides struct is refused at S = 1 too
    refused(call, "S = 1 with a NULL strides struct")


# ------------------------------------------------------------------------------------------------ the compiled kernels
GATE = "<evac::AdamHeader const*, evac::TfgLearnerStrides>"
TWINS = {"k_tf_encode" + GATE: "k_tf_encode<evac::AdamHeader const*>", "k_tf_dy" + GATE: "k_tf_dy<evac::AdamHeader const*>",
         "k_tf_backward" + GATE: "k_tf_backward<evac::AdamHeader const*>", "k_tf_finish" + GATE: "k_tf_finish<evac::AdamHeader const*>",
         "k_adam_tf_population": "k_adam_tf("}


def test_the_new_unit_holds_five_kernels_with_no_scratch(monkeypatch):
    monkeypatch.setattr(kernel_meta, "FIELDS", kernel_meta.FIELDS + ("group_segment_fixed_size",))
    mine = kernel_meta.kernel_resources(UNIT)
    lone = kernel_meta.kernel_resources("evac_transformer_update_api.hip")
    stems = sorted(n.split("(")[0].replace("void ", "") for n in mine)
    assert stems == sorted("evac::" + k for k in TWINS), stems
    # no actor-critic kernel and no lone kernel is defined a second time: the middle of a step is evac_population_api.hip's
    assert not any(t in n for n in mine for t in ("k_rpo", "k_population", "k_gae", "k_adam_tf("))
    assert len(lone) == 15                                          # evac_transformer_update_api.hip's own kernels are as they were
    for name, k in mine.items():
        twin = next(v for n, v in lone.items() if TWINS[next(s for s in TWINS if s in name)] in n)
        print(f"{name}: vgpr {k['vgpr_count']} (twin {twin['vgpr_count']}), sgpr {k['sgpr_count']} (twin {twin['sgpr_count']}), "
              f"sgpr spills {k['sgpr_spill_count']} (twin {twin['sgpr_spill_count']}), LDS {k['group_segment_fixed_size']} B")
        assert k["private_segment_fixed_size"] == 0 and k["vgpr_spill_count"] == 0, (name, k)
        assert k["group_segment_fixed_size"] == twin["group_segment_fixed_size"], (name, k, twin)      # the twin's LDS plan
        if "k_tf_backward" in name:
            assert 0 < k["group_segment_fixed_size"] <= 64 * 1024, (name, k)
    design = open(os.path.join(ROOT, "DESIGN.md")).read()
    assert "4.20" in design and "evac_transformer_population_update_api.hip: 5 kernels" in design
    for stem in ("k_tf_encode", "k_tf_dy", "k_tf_backward", "k_tf_finish", "k_adam_tf_population", "TfgLearnerStrides", "TfAdamStrides"):
        assert stem in design, stem


# ------------------------------------------------------------------------------------------------ the Python faces
def test_the_new_faces_refuse_what_they_should():
    import evacuation_amd
    from evacuation_amd import population
    from evacuation_amd.population import (DeepSetsPopulation, PopulationTrainer, TransformerPopulation, TransformerPopulationAdam,
                                           transformer_update_population)
    from evacuation_amd.policy import TransformerActorCritic, all_tensors
    from evacuation_amd.trainer import RPOTrainingConfig, TransformerAdam
    for name in ("TransformerPopulationAdam", "transformer_update_population"):
        assert name in evacuation_amd.__all__ and getattr(evacuation_amd, name) is getattr(population, name)
    tf = TransformerPopulation(72, 10, [1, 2], device="cpu")
    ds = DeepSetsPopulation(36, 10, [1, 2], device="cpu")
    cfg = RPOTrainingConfig(num_envs=4, num_steps=8, total_timesteps=64, num_minibatches=2)
    env = SimpleNamespace(num_envs=8)
    # the optimiser: anything but a TransformerPopulation
    for other in (ds, SimpleNamespace(num_learners=1, device=torch.device("cpu"), tensors=[], nets=[]), tf.nets[0]):
        with pytest.raises(ValueError, match="TransformerPopulationAdam: a TransformerPopulation is expected"):
            TransformerPopulationAdam(other)
    assert issubclass(TransformerPopulationAdam, population.PopulationAdam)
    # TransformerAdam(storage=): the count of the network's tensors, 45 here
    net = TransformerActorCritic(72, 10)
    count = len(all_tensors(net))
    assert count == 45
    header, moments = torch.zeros(8, dtype=torch.int64), [torch.zeros_like(p) for p in all_tensors(net)]
    for m, v in ((moments[:13], moments[:13]), (moments[:29], moments), (moments, moments[:44]), (moments + moments[:1], moments)):
        with pytest.raises(ValueError, match="`storage` is \\(header, 45 exp_avg, 45 exp_avg_sq\\)"):
            TransformerAdam(net, storage=(header, m, v))
    with pytest.raises(ValueError, match="`storage`"):
        TransformerAdam(net, storage=(header, moments))
    one = TransformerActorCritic(72, 10, num_blocks=1)
    with pytest.raises(ValueError, match="29 exp_avg"):
        TransformerAdam(one, storage=(header, moments, moments))
    # the update
    with pytest.raises(ValueError, match="transformer_update_population: a TransformerPopulation is expected"):
        transformer_update_population(ds, {}, None, cfg, None)
    with pytest.raises(ValueError, match="a TransformerPopulationAdam is expected, got SimpleNamespace"):
        transformer_update_population(tf, {}, None, cfg, SimpleNamespace())
    group = lambda lr: SimpleNamespace(param_groups=[{"lr": lr, "max_grad_norm": 0.5}])
    opt = TransformerPopulationAdam.__new__(TransformerPopulationAdam)          # (its state needs a device; its learners' groups do not)
    opt.population, opt.learners = tf, [group(3e-4), group(3e-4)]
    with pytest.raises(ValueError, match="sweeps of transformer learners are not built"):
        transformer_update_population(tf, {}, None, [cfg, cfg], opt)
    opt.learners = [group(3e-4), group(1e-3)]
    with pytest.raises(ValueError, match="sweeps of transformer learners are not built"):
        transformer_update_population(tf, {}, None, cfg, opt)
    # the sizer
    build.build_library()
    assert population.population_workspace_bytes(72, 16, 3, transformer=True) == \
        _lib.load().evac_transformer_population_workspace_bytes(72, 16, 3)
    with pytest.raises(ValueError, match="two kinds"):
        population.population_workspace_bytes(72, 16, 3, transformer=True, deepsets=True)
    with pytest.raises(_lib.EvacError):
        population.population_workspace_bytes(72, 16, 65, transformer=True)
    # the trainer
    with pytest.raises(ValueError, match="expected None or \"device_transformer\""):
        PopulationTrainer(env, tf, cfg, optimizer="device")
    for other in (ds, population.PolicyPopulation(72, [1, 2], device="cpu")):
        with pytest.raises(ValueError, match="trains a TransformerPopulation"):
            PopulationTrainer(env, other, cfg, optimizer="device_transformer")
    with pytest.raises(ValueError, match="sweeps of transformer learners are not built"):
        PopulationTrainer(env, tf, [cfg, dataclasses.replace(cfg, learning_rate=1e-3)], optimizer="device_transformer")
    with pytest.raises(ValueError, match="1 configurations for 2 learners"):
        PopulationTrainer(env, tf, [cfg], optimizer="device_transformer")
    with pytest.raises(ValueError, match="2 learners x cfg.num_envs"):
        PopulationTrainer(SimpleNamespace(num_envs=9), tf, cfg, optimizer="device_transformer")
    with pytest.raises(ValueError, match="2 learners x cfg.num_envs"):          # (the same configuration twice is ONE configuration)
        PopulationTrainer(SimpleNamespace(num_envs=9), tf, [cfg, dataclasses.replace(cfg, seed=7)], optimizer="device_transformer")
    wet = TransformerPopulation(72, 10, [1, 2], device="cpu")
    for m in wet.nets[1].embedding.modules():
        if isinstance(m, torch.nn.Dropout):
            m.p = 0.1
    with pytest.raises(ValueError, match="PopulationTrainer: `embedding` has dropout p = 0.1"):      # every learner, not the first alone
        PopulationTrainer(env, wet, cfg, optimizer="device_transformer")


def test_the_default_faces_still_refuse_and_name_the_opt_in():
    from evacuation_amd.population import PopulationAdam, PopulationTrainer, TransformerPopulation
    from evacuation_amd.trainer import RPOTrainingConfig
    pop = TransformerPopulation(72, 10, [1, 2], device="cpu")
    env = SimpleNamespace(num_envs=8)
    cfg = RPOTrainingConfig(num_envs=4, num_steps=8, total_timesteps=64)
    for what, make in (("PopulationTrainer", lambda: PopulationTrainer(env, pop, cfg)), ("PopulationAdam", lambda: PopulationAdam(pop)),
                       ("PopulationTrainer", lambda: PopulationTrainer(env, pop, [cfg, cfg])),
                       ("PopulationTrainer", lambda: PopulationTrainer(env, pop, cfg, optimizer=None))):
        with pytest.raises(ValueError) as e:
            make()
        text = str(e.value)
        assert text.startswith(what + ": the update of transformer learners is not built"), text
        for works in ("policy_rollout_population", "policy_evaluate_population", "PopulationEvaluator",
                      'RPOTrainer(grad_fn=transformer_kernel_grad, optimizer="device_transformer")', "nets[s]",
                      "these two default faces do not take", "TransformerPopulationAdam", "transformer_update_population",
                      'PopulationTrainer(..., optimizer="device_transformer")'):
            assert works in text, (what, works)
