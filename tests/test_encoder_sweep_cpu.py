"""CPU tests of the sweeps of the two encoder leaders (include/evac.h: evac_policy_rollout_sweep_deepsets / _transformer,
evac_deepsets_update_sweep / evac_transformer_update_sweep, evac_deepsets_sweep_workspace_bytes /
evac_transformer_sweep_workspace_bytes; evacuation_amd.population.deepsets_update_sweep, transformer_update_sweep,
PopulationTrainer(encoder_sweep=True)): the symbols, the sizers, the update entries' refusals with no device present (no pointer is
ever followed: they are made-up addresses), the build's sources, the compiled kernels of the two new translation units and the
Python faces on the CPU."""
import ctypes as C
import dataclasses
import os
import re
from types import SimpleNamespace

import pytest
import torch

from evacuation_amd import _lib, build
from tests import kernel_meta
from tests import test_deepsets_population_cpu as DS
from tests import test_transformer_population_update_cpu as TF

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BAD, UNSUPPORTED = _lib.ERR_INVALID_ARGUMENT, _lib.ERR_UNSUPPORTED
ENCODERS = ("deepsets", "transformer")
UNITS = {"deepsets": "evac_deepsets_sweep_api.hip", "transformer": "evac_transformer_sweep_api.hip"}
TABLE_BYTES = 64 * 8 + 64 * 8 + 64 * 4 + 8      # evac::LearnerSteps: lr, target_kl (double), max_norm (float), the targets' mask


def round256(n):
    return (n + 255) // 256 * 256


@pytest.fixture(scope="module")
def lib():
    build.build_library()
    return _lib.load()


def test_symbols_are_declared_exported_and_bound(lib):
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "evac.h")).read(), flags=re.S)
    for enc in ENCODERS:
        for name, twin, more in ((f"evac_policy_rollout_sweep_{enc}", f"evac_policy_rollout_population_{enc}", 1),
                                 (f"evac_{enc}_update_sweep", f"evac_{enc}_update_population", -1)):
            decl, base = (re.search(rf"int {n}\((.*?)\);", text, re.S) for n in (name, twin))
            assert decl and base and name in _lib.SIGNATURES, name
            params = decl.group(1).split(",")
            fn = getattr(lib, name)
            assert len(fn.argtypes) == len(params) == len(base.group(1).split(",")) + more and fn.restype is C.c_int, name
            at = -2 if more == 1 else -4         # in front of the stream; in place of use_target_kl, target_kl
            assert "const evac_learner_hyper_t* hypers" in params[at], (name, params[at])
            assert fn.argtypes[at] is C.POINTER(_lib.EvacLearnerHyper), name
        sizer = f"evac_{enc}_sweep_workspace_bytes"
        assert re.search(rf"int64_t {sizer}\(int32_t \w+, int64_t \w+, int32_t \w+\);", text) and sizer in _lib.SIGNATURES
        fn = getattr(lib, sizer)
        assert fn.restype is C.c_int64 and len(fn.argtypes) == 3
    assert lib.evac_version() == _lib.VERSION == 150


def test_the_units_are_built_before_the_capture_unit():
    names = [os.path.basename(s) for s in build.SOURCES]
    assert names[-1] == "evac_capture_api.hip"
    at = names.index("evac_transformer_population_update_api.hip")
    assert names[at + 1:at + 3] == [UNITS["deepsets"], UNITS["transformer"]] and at + 3 == len(names) - 1
    for f in list(UNITS.values()) + ["evac_encoder_sweep.h", "evac_sweep_host.h", "evac_sweep_args.h"]:
        assert os.path.join(build.CSRC, f) in build.DEPENDS, f


@pytest.mark.parametrize("enc", ENCODERS)
def test_workspace_bytes(lib, enc):
    sweep, pop = getattr(lib, f"evac_{enc}_sweep_workspace_bytes"), getattr(lib, f"evac_{enc}_population_workspace_bytes")
    assert round256(TABLE_BYTES) == 1536
    for D, M, S in ((36, 70, 3), (372, 192, 8), (384, 1024, 64)):
        assert pop(D, M, S) > 0 and pop(D, M, S) % 256 == 0
        assert sweep(D, M, S) == pop(D, M, S) + round256(TABLE_BYTES), (D, M, S)
    for bad in ((0, 64, 2), (397, 64, 2), (6, 0, 2), (6, -1, 2), (36, 64, 0), (36, 64, -1), (36, 64, 65)):
        assert pop(*bad) == BAD and sweep(*bad) == BAD, bad


# ------------------------------------------------------------------------------------------------ refusals
class SweepLib:
    """The population's test calls (tests/test_deepsets_population_cpu.Update, tests/test_transformer_population_update_cpu.Update)
    sent to the sweep entry: `hypers` in place of use_target_kl, target_kl."""

    def __init__(self, lib, hypers):
        self.lib, self.hypers = lib, hypers

    def __getattr__(self, name):
        assert name.endswith("_update_population"), name
        entry = getattr(self.lib, name.replace("_update_population", "_update_sweep"))
        return lambda *a: entry(*a[:-5], self.hypers, *a[-3:])


@pytest.mark.parametrize("enc", ENCODERS)
def test_update_refusals_without_a_device(lib, enc):
    """Every refusal is decided on the host: the pointers are made up, and a call that got past the checks would follow them.  The
    population's refusals come first, in the population's order; `hypers` is looked at last."""
    Update = (DS if enc == "deepsets" else TF).Update
    good = _lib.learner_hypers(2)

    def refused(call, hypers, why, code=BAD):
        assert call(SweepLib(lib, hypers)) == code, why

    # the population's own, with acceptable values
    for S in (0, 65):
        refused(Update(S=S), _lib.learner_hypers(max(S, 1) if S < 65 else 64), f"n_learners {S}")
    for name in ("param_strides", "enc_param_strides", "grad_strides", "enc_grad_strides", "moment_strides", "enc_moment_strides",
                 "pol", "enc", "params", "enc_params", "grads", "enc_grads", "cfg", "adam", "state"):
        call = Update()
        call.null.add(name)
        refused(call, good, f"NULL {name}")
    for stride in (56, 68):
        call = Update()
        call.header_stride = stride
        refused(call, good, f"header stride {stride}")
    call = Update()
    call.workspace = TF.FAKE + 8
    refused(call, good, "a misaligned workspace")
    refused(Update(epochs=0), good, "n_epochs 0")
    refused(Update(B_l=0), good, "learner_batch_size 0")
    refused(Update(M=1), good, "one sample with norm_adv")
    for flag in ("seeds", "counters"):
        call = Update()
        setattr(call, flag, False)
        refused(call, good, f"NULL {flag}")
    call = Update()
    call.strides[1].actor_w1 = 64 * 36 - 1
    refused(call, good, "a policy stride below its tensor")
    if enc == "transformer":
        refused(Update(dm=3, D=3 * 65), good, "65 tokens", UNSUPPORTED)
        # the order: the population's refusals before the learners' values
        call = Update()
        call.enc.num_heads = 4
        refused(call, None, "num_heads 4 and NULL hypers: the encoder first", UNSUPPORTED)
        call = Update()
        call.enc.num_blocks = 3
        refused(call, _lib.learner_hypers(2, learning_rate=[1e-3, float("inf")]), "num_blocks 3 and a refused rate: the encoder first",
                UNSUPPORTED)
    else:
        call = Update()
        call.enc_strides[0].rho_w = 36 * 24 + 2
        refused(call, good, "rho_w's stride no multiple of 4 floats")
    # then the learners' values: everything else acceptable
    refused(Update(), None, "NULL hypers")
    for field, value in (("learning_rate", float("nan")), ("learning_rate", float("inf")), ("gamma", float("nan")),
                         ("max_grad_norm", 0.0), ("clip_coef", -0.1), ("rpo_alpha", float("nan"))):
        for s in range(2):
            column = [HYPER_OK[field]] * 2
            column[s] = value
            refused(Update(), _lib.learner_hypers(2, **{field: column}), f"{field} = {value} of learner {s}")
    nan_target = _lib.learner_hypers(2)
    nan_target[1].use_target_kl, nan_target[1].target_kl = 1, float("nan")
    refused(Update(), nan_target, "a NaN target in use")


HYPER_OK = dict(_lib.HYPER_DEFAULTS)


@pytest.mark.parametrize("enc", ENCODERS)
def test_collection_refuses_without_a_handle(lib, enc):
    entry = getattr(lib, f"evac_policy_rollout_sweep_{enc}")
    assert entry(None, 2, None, None, None, None, 8, *[None] * 11, 0.99, 10.0, 10.0, 1e-8, None, None) == BAD      # (a NULL handle)


# ------------------------------------------------------------------------------------------------ the compiled kernels
COLLECT = {"deepsets": ("k_collect_sweep_deepsets", "evac_deepsets_population_api.hip", "k_collect_population_deepsets<true, "),
           "transformer": ("k_collect_sweep_transformer", "evac_transformer_population_api.hip", "k_collect_population_transformer<true, ")}
ADAM = {"deepsets": "k_adam_set_sweep", "transformer": "k_adam_tf_sweep"}
ENCODER_KERNELS = {"deepsets": ("k_set_encode", "k_set_backward", "k_set_finish"),
                   "transformer": ("k_tf_encode", "k_tf_dy", "k_tf_backward", "k_tf_finish")}


@pytest.mark.parametrize("enc", ENCODERS)
def test_the_new_kernels_have_no_scratch_and_their_twins_lds(monkeypatch, enc):
    monkeypatch.setattr(kernel_meta, "FIELDS", kernel_meta.FIELDS + ("group_segment_fixed_size", "kernarg_segment_size"))
    mine = kernel_meta.kernel_resources(UNITS[enc])
    stem, twin_unit, twin_stem = COLLECT[enc]
    twins = kernel_meta.kernel_resources(twin_unit)
    stems = sorted(set(n.split("(")[0].replace("void ", "").split("<")[0] for n in mine))
    assert stems == sorted("evac::" + k for k in (stem, ADAM[enc], "k_learner_steps_table") + ENCODER_KERNELS[enc]), stems
    # no actor-critic kernel and no population kernel is defined a second time
    assert not any(t in n for n in mine for t in ("k_rpo", "k_population", "k_sweep_grad", "k_sweep_finish", "k_gae", "_population"))
    collect = {n: k for n, k in mine.items() if stem in n}
    assert len(collect) == 2 and any(stem + "<true>" in n for n in collect) and any(stem + "<false>" in n for n in collect)
    for name, k in list(collect.items()) + [(n, k) for n, k in mine.items() if ADAM[enc] in n or "k_learner_steps_table" in n]:
        print(f"{name.split('(')[0]}: vgpr {k['vgpr_count']}, sgpr {k['sgpr_count']}, sgpr spills {k['sgpr_spill_count']}, "
              f"LDS {k['group_segment_fixed_size']} B, arguments {k['kernarg_segment_size']} B")
        assert k["private_segment_fixed_size"] == 0 and k["vgpr_spill_count"] == 0, (name, k)
        assert k["kernarg_segment_size"] <= 4096, (name, k)
    for name, k in collect.items():
        DEF = "true" if stem + "<true>" in name else "false"
        twin = next(v for n, v in twins.items() if twin_stem + DEF + ">" in n)
        assert k["vgpr_count"] <= 128, (name, k)
        assert 0 < k["group_segment_fixed_size"] <= twin["group_segment_fixed_size"] <= 160 * 1024, (name, k, twin)
    # the encoder's own kernels are the population's instantiations: the learner as blockIdx.y, no hyperparameter read
    for name, k in mine.items():
        if any(e in name for e in ENCODER_KERNELS[enc]):
            assert "evac::AdamHeader const*" in name and "LearnerStrides" in name, name
            assert k["private_segment_fixed_size"] == 0 and k["vgpr_spill_count"] == 0, (name, k)
    source = open(os.path.join(build.CSRC, UNITS[enc])).read()
    assert source.count("static_assert(") >= 3 and source.count("<= 4096") >= 2 and "<= 160 * 1024" in source
    assert "sizeof(evac::LearnerGammas) <= 4096" in source


def test_design_records_the_sweep():
    design = open(os.path.join(ROOT, "DESIGN.md")).read()
    assert "4.22" in design
    for word in ("k_collect_sweep_deepsets", "k_collect_sweep_transformer", "k_adam_set_sweep", "k_adam_tf_sweep", "k_learner_steps_table",
                 "1896", "1096", "1288", "encoder_sweep=True"):
        assert word in design, word
    assert os.path.exists(os.path.join(ROOT, "profiles", "kernel_asm_diff_encoder_sweep.txt"))


# ------------------------------------------------------------------------------------------------ the Python faces
def test_the_python_faces_without_a_device():
    import evacuation_amd
    from evacuation_amd import population
    from evacuation_amd.population import (DeepSetsPopulation, PolicyPopulation, PopulationTrainer, TransformerPopulation,
                                           deepsets_update_sweep, transformer_update_sweep)
    from evacuation_amd.trainer import RPOTrainingConfig
    for name in ("deepsets_update_sweep", "transformer_update_sweep"):
        assert name in evacuation_amd.__all__ and getattr(evacuation_amd, name) is getattr(population, name)
    tf = TransformerPopulation(72, 10, [1, 2], device="cpu")
    ds = DeepSetsPopulation(36, 10, [1, 2], device="cpu")
    lin = PolicyPopulation(36, [1, 2], device="cpu")
    cfg = RPOTrainingConfig(num_envs=4, num_steps=8, total_timesteps=64, num_minibatches=2)
    cfgs = [cfg, dataclasses.replace(cfg, learning_rate=1e-3, gamma=0.9)]
    env = SimpleNamespace(num_envs=8)
    # the keyword with a PolicyPopulation: the default path already sweeps
    with pytest.raises(ValueError, match="the default path already sweeps"):
        PopulationTrainer(env, lin, cfgs, encoder_sweep=True)
    # a structural field that differs
    for pop, kw in ((ds, {}), (tf, {"optimizer": "device_transformer"})):
        with pytest.raises(ValueError, match="num_steps = 16 of learner 1 differs from learner 0's 8"):
            PopulationTrainer(env, pop, [cfg, dataclasses.replace(cfg, num_steps=16)], encoder_sweep=True, **kw)
        with pytest.raises(ValueError, match="1 configurations for 2 learners"):
            PopulationTrainer(env, pop, [cfg], encoder_sweep=True, **kw)
        with pytest.raises(ValueError, match="2 learners x cfg.num_envs"):      # past every refusal of the configurations
            PopulationTrainer(SimpleNamespace(num_envs=9), pop, cfgs, encoder_sweep=True, **kw)
    # a transformer population still asks for its optimiser by name, and without the keyword differing configurations stay refused
    with pytest.raises(ValueError, match="the update of transformer learners is not built into"):
        PopulationTrainer(env, tf, cfgs, encoder_sweep=True)
    for pop, kw, kind in ((ds, {}, "deep-sets"), (tf, {"optimizer": "device_transformer"}, "transformer")):
        with pytest.raises(ValueError, match=f"sweeps of {kind} learners are not built.*encoder_sweep=True"):
            PopulationTrainer(env, pop, cfgs, **kw)
    # dropout other than 0
    wet = TransformerPopulation(72, 10, [1, 2], device="cpu")
    for m in wet.nets[1].embedding.modules():
        if isinstance(m, torch.nn.Dropout):
            m.p = 0.1
    with pytest.raises(ValueError, match="PopulationTrainer: `embedding` has dropout p = 0.1"):
        PopulationTrainer(env, wet, cfgs, optimizer="device_transformer", encoder_sweep=True)
    opt = population.TransformerPopulationAdam.__new__(population.TransformerPopulationAdam)
    opt.population, opt.learners = wet, []
    with pytest.raises(ValueError, match="transformer_update_sweep: `embedding` has dropout p = 0.1"):
        transformer_update_sweep(wet, {}, None, cfgs, opt)
    # the update's faces: the kind of population and of optimiser
    with pytest.raises(ValueError, match="deepsets_update_sweep: a DeepSetsPopulation is expected"):
        deepsets_update_sweep(lin, {}, None, cfgs, None)
    with pytest.raises(ValueError, match="transformer_update_sweep: a TransformerPopulation is expected"):
        transformer_update_sweep(ds, {}, None, cfgs, None)
    with pytest.raises(ValueError, match="a TransformerPopulationAdam is expected, got SimpleNamespace"):
        transformer_update_sweep(tf, {}, None, cfgs, SimpleNamespace())
    # the sizer
    build.build_library()
    for kind in ENCODERS:
        assert population.population_workspace_bytes(72, 16, 3, sweep=True, **{kind: True}) == \
            getattr(_lib.load(), f"evac_{kind}_sweep_workspace_bytes")(72, 16, 3)
    assert population.population_workspace_bytes(72, 16, 3, sweep=True) == population.population_workspace_bytes(72, 16, 3)
    # the env's face exists on both envs
    import evacuation_amd as ea
    assert callable(ea.BatchedEvacuationEnv.policy_rollout_sweep) and callable(ea.NormalizedVectorEnv.policy_rollout_sweep)
