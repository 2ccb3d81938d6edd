"""CPU checks of the transformer leader's population form on a handle's envs (evac_policy_rollout_population_transformer,
evac_policy_evaluate_population_transformer, population.TransformerPopulation): the ABI, the two units' place in
the build, what the compiler made of their kernels, the stacked population object, and what stays refused."""
import ctypes as C
import os
import re
from types import SimpleNamespace

import pytest
import torch

from evacuation_amd import _lib, build
from evacuation_amd.policy import TransformerActorCritic, all_tensors
from tests import kernel_meta

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
COLLECT_UNIT, EVALUATE_UNIT = "evac_transformer_population_api.hip", "evac_transformer_population_evaluate_api.hip"
COLLECT, EVALUATE = "evac_policy_rollout_population_transformer", "evac_policy_evaluate_population_transformer"
FLAGS = [f"<{n}, {d}>" for n in ("true", "false") for d in ("true", "false")]           # <NORM, DEF>
CPU = torch.device("cpu")


@pytest.fixture(scope="module")
def lib():
    build.build_library()
    return _lib.load()


# ------------------------------------------------------------------------------------------------ the ABI
def declared(entry):
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "evac.h")).read(), flags=re.S)
    m = re.search(r"\bint\s+" + entry + r"\s*\(([^;]*)\)\s*;", text)
    assert m, f"the declaration of {entry} in evac.h"
    return [p.strip() for p in m.group(1).split(",")]


def test_entries_are_declared_exported_and_bound(lib):
    front = [C.c_void_p, C.c_int32, C.POINTER(_lib.EvacMlpPolicy), C.POINTER(_lib.EvacMlpPolicyStrides), C.POINTER(_lib.EvacTransformer),
             C.POINTER(_lib.EvacTransformerStrides)]
    sibling = {COLLECT: "evac_policy_rollout_population_deepsets", EVALUATE: "evac_policy_evaluate_population_deepsets"}
    for entry, count in ((COLLECT, 23), (EVALUATE, 16)):
        params = declared(entry)
        assert len(params) == count == len(declared(sibling[entry])), entry
        assert "evac_mlp_policy_strides_t" in params[3] and "evac_transformer_t" in params[4] and "evac_transformer_strides_t" in params[5]
        assert "stream" in params[-1]
        res, args = _lib.SIGNATURES[entry]
        assert res is C.c_int and len(args) == count and args[:6] == front and args[-1] is C.c_void_p, entry
        # behind the two encoder arguments the entry is its deep-sets sibling
        assert args[6:] == _lib.SIGNATURES[sibling[entry]][1][6:], entry
        assert [p.split()[-1].lstrip("*") for p in params[6:]] == [p.split()[-1].lstrip("*") for p in declared(sibling[entry])[6:]], entry
        assert getattr(lib, entry) is not None
    assert "n_steps" in declared(COLLECT)[6] and "agent" in declared(EVALUATE)[6] and "shared_episodes" in declared(EVALUATE)[7]
    assert lib.evac_version() == _lib.VERSION == 150
    # the strides' structs: 16 int64 per block in evac_transformer_block_t's order, two blocks
    assert [f for f, _ in _lib.EvacTransformerBlockStrides._fields_] == [f for f, _ in _lib.EvacTransformerBlock._fields_]
    assert C.sizeof(_lib.EvacTransformerBlockStrides) == 16 * 8 and C.sizeof(_lib.EvacTransformerStrides) == 2 * 16 * 8
    header = open(os.path.join(ROOT, "include", "evac.h")).read()
    m = re.search(r"typedef struct evac_transformer_block_strides\s*\{([^}]*)\}", re.sub(r"/\*.*?\*/", "", header, flags=re.S))
    assert m and [w.strip() for w in m.group(1).replace("int64_t", "").replace(";", "").split(",")] == \
        [f for f, _ in _lib.EvacTransformerBlock._fields_]


def test_a_null_handle_is_refused_strides_or_no_strides(lib):
    pol, st = _lib.EvacMlpPolicy(), _lib.EvacMlpPolicyStrides()
    enc, est = _lib.EvacTransformer(), _lib.EvacTransformerStrides()
    with_, without = [C.byref(pol), C.byref(st), C.byref(enc), C.byref(est)], [None] * 4
    for nets in (with_, without):
        assert getattr(lib, COLLECT)(None, 2, *nets, 1, *[None] * 11, 0.99, 1.0, 100.0, 1e-8, None) == _lib.ERR_INVALID_ARGUMENT
        assert getattr(lib, EVALUATE)(None, 2, *nets, 0, 1, 1, 1, None, None, None, 1.0, 1e-8, None) == _lib.ERR_INVALID_ARGUMENT


# ------------------------------------------------------------------------------------------------ the build
def test_the_units_are_built_before_the_recording_evaluation():
    names = [os.path.basename(s) for s in build.SOURCES]
    assert names[-1] == "evac_capture_api.hip"
    for unit in (COLLECT_UNIT, EVALUATE_UNIT):
        assert names.count(unit) == 1 and names.index(unit) > names.index("evac_deepsets_population_evaluate_api.hip")
        assert os.path.join(build.CSRC, unit) in build.DEPENDS
    assert os.path.join(build.CSRC, "evac_transformer_population.h") in build.DEPENDS
    for unit in (COLLECT_UNIT, EVALUATE_UNIT):       # a kernel-argument segment and a CU's LDS, asserted where the kernels are launched
        text = open(os.path.join(build.CSRC, unit)).read()
        assert text.count("static_assert(") >= 2 and "<= 4096" in text and "160 * 1024" in text, unit


# ------------------------------------------------------------------------------------------------ the kernels' resources
# private_segment_fixed_size of the new kernels by their <NORM, DEF>, as measured
COLLECT_SCRATCH = {"<true, true>": 0, "<true, false>": 0, "<false, true>": 0, "<false, false>": 0}
EVALUATE_SCRATCH = {"<true, true>": 0, "<true, false>": 0, "<false, true>": 0, "<false, false>": 0}


@pytest.fixture(scope="module")
def resources():
    fields, kernel_meta.FIELDS = kernel_meta.FIELDS, tuple(kernel_meta.FIELDS) + ("group_segment_fixed_size",)
    try:
        return {unit: kernel_meta.kernel_resources(unit) for unit in (COLLECT_UNIT, EVALUATE_UNIT, "evac_transformer_api.hip")}
    finally:
        kernel_meta.FIELDS = fields


def stem(name):
    return name.split("(")[0].replace("void ", "")


UNITS = [(COLLECT_UNIT, "evac::k_collect_population_transformer", "k_policy_rollout_transformer<", COLLECT_SCRATCH),
         (EVALUATE_UNIT, "evac::k_evaluate_population_transformer", "k_policy_evaluate_transformer<", EVALUATE_SCRATCH)]


@pytest.mark.parametrize("unit,kernel,twin,pinned", UNITS)
def test_a_unit_holds_its_four_kernels_within_the_lone_kernels_budget(resources, unit, kernel, twin, pinned):
    """The learner's shift leaves the encoder's arguments in the kernel-argument segment: no array in scratch, and none of the
    spilled dwords of the lone twins either (tests/test_transformer_cpu.py pins 8 B and 12 B there) -- the measured sizes, all
    0, are pinned, and stay within the 16 bytes tests/test_evaluate_capture_cpu.py allows on top of the twin."""
    mine, lone_all = resources[unit], resources["evac_transformer_api.hip"]
    assert len(lone_all) == 8                                        # evac_transformer_api.hip's own kernels are as they were
    lone = {n: k for n, k in lone_all.items() if twin in n}
    assert sorted(stem(n) for n in mine) == sorted(kernel + f for f in FLAGS), sorted(mine)
    assert len(lone) == 4
    for name, k in mine.items():
        f = next(f for f in FLAGS if f in name)
        t = next(v for n, v in lone.items() if f in n)
        print(f"\n{stem(name)}: {k}\n    lone twin: {t}")
        assert k["vgpr_count"] <= 128, (name, k)
        assert k["private_segment_fixed_size"] <= t["private_segment_fixed_size"] + 16, (name, k, t)
        assert k["private_segment_fixed_size"] == pinned[f], (name, k)
        assert 0 < k["group_segment_fixed_size"] <= t["group_segment_fixed_size"] <= 160 * 1024, (name, k, t)   # (the shifts need no LDS)
    design = open(os.path.join(ROOT, "DESIGN.md")).read()
    assert kernel.replace("evac::", "") in design and COLLECT in design and EVALUATE in design


@pytest.mark.parametrize("unit,kernel,twin,pinned", UNITS)
def test_no_kernel_of_a_unit_spills_a_vector_register(resources, unit, kernel, twin, pinned):
    """``vgpr_spill_count == 0`` in all four kernels of a unit.  The step body is at the limit of 128 registers (two of the lone
    kernels spill one and two); the learner's encoder forms its lane and row addresses anew at every call
    (TransformerLearnerTensors::fresh) instead of carrying them through the step loop, which is what leaves room."""
    for name, k in resources[unit].items():
        assert k["vgpr_spill_count"] == 0, (stem(name), k)


# ------------------------------------------------------------------------------------------------ TransformerPopulation
def shapes(D, dm, blocks):
    H, F = 64, 96
    mlp = [(H, D), (H,), (H, H), (H,), (2, H), (2,), (1, 2), (H, D), (H,), (H, H), (H,), (1, H), (1,)]
    block = [(3 * dm, dm), (3 * dm,)] * 3 + [(dm, 3 * dm), (dm,), (F, dm), (F,), (dm, F), (dm,)] + [(dm,)] * 4
    return mlp + block * blocks


@pytest.mark.parametrize("N,dm,blocks,resid", [(10, 6, 2, False), (4, 3, 1, True)])
def test_population_is_its_freshly_seeded_nets_stacked(N, dm, blocks, resid):
    from evacuation_amd.population import TransformerPopulation
    D, seeds = (N + 2) * dm, [11, 18, 25]
    torch.manual_seed(99)
    before = torch.get_rng_state()
    pop = TransformerPopulation(D, N, seeds, device="cpu", num_blocks=blocks, use_resid=resid)
    assert torch.equal(torch.get_rng_state(), before)               # the caller's generator is where it was
    S = len(seeds)
    assert pop.num_learners == S and len(pop.nets) == S and (pop.token_dim, pop.num_blocks, pop.use_resid) == (dm, blocks, resid)
    assert len(pop.tensors) == len(pop.grads) == 13 + 16 * blocks == (45 if blocks == 2 else 29)
    assert [tuple(t.shape) for t in pop.tensors] == [(S,) + s for s in shapes(D, dm, blocks)]
    assert not hasattr(pop, "embedding") and not hasattr(pop, "deep_sets")
    for s, seed in enumerate(seeds):
        torch.manual_seed(seed)
        fresh = TransformerActorCritic(D, N, num_blocks=blocks, use_resid=resid)
        net = pop.nets[s]
        assert isinstance(net, TransformerActorCritic) and len(list(net.parameters())) == len(pop.tensors)
        assert all(m.p == 0.0 for m in net.modules() if isinstance(m, torch.nn.Dropout))
        for i, (p, q) in enumerate(zip(all_tensors(net), all_tensors(fresh))):
            assert torch.equal(p.view(torch.int32), q.view(torch.int32)), (s, i)
            assert p.data_ptr() == pop.tensors[i][s].data_ptr() and p.grad.data_ptr() == pop.grads[i][s].data_ptr(), (s, i)
            assert p.is_contiguous() and tuple(p.shape) == tuple(pop.tensors[i].shape[1:])
    # the strides and the structs: learner 0's tensors, a row further per learner
    sizes = [t[0].numel() for t in pop.tensors]
    assert [getattr(pop.strides, f) for f, _ in _lib.EvacMlpPolicyStrides._fields_] == sizes[:13]
    fields = [f for f, _ in _lib.EvacTransformerBlockStrides._fields_]
    for b in range(2):
        got = [getattr(pop.encoder_strides.blocks[b], f) for f in fields]
        assert got == (sizes[13 + 16 * b:29 + 16 * b] if b < blocks else [0] * 16), b
    pol, enc = pop.policy_struct(), pop.encoder_struct()
    assert (pol.obs_dim, pol.hidden) == (D, 64)
    assert [getattr(pol, f) for f, _ in _lib.EvacMlpPolicy._fields_[2:]] == [t.data_ptr() for t in pop.tensors[:13]]
    assert (enc.elem_dim, enc.num_blocks, enc.num_heads, enc.dim_feedforward, enc.use_resid) == (dm, blocks, 3, 96, int(resid))
    for b in range(blocks):
        assert [getattr(enc.blocks[b], f) for f in fields] == [t.data_ptr() for t in pop.tensors[13 + 16 * b:29 + 16 * b]], b
    # the stack IS the nets: a change of a row is the net's, and the net computes with it
    x = torch.randn(5, D)
    v0, other = pop.nets[1].get_value(x).detach().clone(), pop.nets[0].get_value(x).detach().clone()
    assert tuple(v0.shape) == (5, 1) and torch.isfinite(v0).all()
    with torch.no_grad():
        pop.tensors[12][1] += 2.0                                   # critic_b3 of learner 1
        pop.tensors[13 + 15][1] += 0.5                              # the first block's norm2_b
    assert torch.equal(pop.nets[1].critic[4].bias, pop.tensors[12][1])
    assert torch.equal(pop.nets[1].embedding[0].norm2.bias, pop.tensors[28][1])
    assert not torch.equal(pop.nets[1].get_value(x), v0)
    assert torch.equal(pop.nets[0].get_value(x), other)            # ... and nobody else's
    pop.nets[2].get_value(x).sum().backward()                       # autograd accumulates into the gradients' row
    assert float(pop.grads[12][2].abs().sum()) > 0 and float(pop.grads[12][0].abs().sum()) == 0
    a, lp, ent, v = pop.nets[0].get_action_and_value(x)
    assert tuple(a.shape) == (5, 2) and tuple(lp.shape) == (5,) and tuple(v.shape) == (5, 1)


def test_population_refuses_what_it_should():
    import evacuation_amd
    from evacuation_amd.population import TransformerPopulation
    assert evacuation_amd.TransformerPopulation is TransformerPopulation and "TransformerPopulation" in evacuation_amd.__all__
    with pytest.raises(ValueError, match="0 learners"):
        TransformerPopulation(72, 10, [], device="cpu")
    with pytest.raises(ValueError, match="65 learners"):
        TransformerPopulation(72, 10, list(range(65)), device="cpu")
    with pytest.raises(ValueError, match="whole number of floats"):
        TransformerPopulation(71, 10, [1, 2], device="cpu")
    with pytest.raises(ValueError, match="num_blocks 3"):
        TransformerPopulation(72, 10, [1], device="cpu", num_blocks=3)
    with pytest.raises(ValueError, match="N <= 62"):
        TransformerPopulation(65 * 6, 63, [1], device="cpu")
    assert TransformerPopulation(72, 10, list(range(64)), device="cpu", num_blocks=1).num_learners == 64


def test_the_update_of_transformer_learners_is_refused_by_name():
    from evacuation_amd.population import PopulationAdam, PopulationTrainer, TransformerPopulation
    from evacuation_amd.trainer import RPOTrainingConfig
    pop = TransformerPopulation(72, 10, [1, 2], device="cpu")
    env = SimpleNamespace(num_envs=8)
    cfg = RPOTrainingConfig(num_envs=4, num_steps=8, total_timesteps=64)
    for what, make in (("PopulationTrainer", lambda: PopulationTrainer(env, pop, cfg)), ("PopulationAdam", lambda: PopulationAdam(pop)),
                       ("PopulationTrainer", lambda: PopulationTrainer(env, pop, [cfg, cfg]))):
        with pytest.raises(ValueError) as e:
            make()
        text = str(e.value)
        assert text.startswith(what + ": the update of transformer learners is not built"), text
        for works in ("policy_rollout_population", "policy_evaluate_population", "PopulationEvaluator",
                      'RPOTrainer(grad_fn=transformer_kernel_grad, optimizer="device_transformer")', "nets[s]"):
            assert works in text, (what, works)


def test_everything_else_with_an_attention_encoder_stays_refused_by_name():
    """Only a real TransformerPopulation takes the new path: a bare network, or a stand-in that holds such networks (with
    encoder strides or without), is refused as before and before `self` is touched."""
    from evacuation_amd import population
    from evacuation_amd.evaluation import PopulationEvaluator
    from evacuation_amd.population import PopulationAdam, PopulationTrainer, TransformerPopulation
    from evacuation_amd.trainer import RPOTrainingConfig
    from evacuation_amd.vector_env import BatchedEvacuationEnv
    pop = TransformerPopulation(72, 10, [1, 2], device="cpu")
    tf = TransformerActorCritic(72, 10)
    cfg = RPOTrainingConfig(num_envs=4, num_steps=8, total_timesteps=64)
    shaped = SimpleNamespace(num_learners=2, nets=[tf, tf], strides=pop.strides, encoder_strides=pop.encoder_strides)
    views = SimpleNamespace(num_learners=2, nets=pop.nets, strides=pop.strides, encoder_strides=pop.encoder_strides,
                            encoder_struct=pop.encoder_struct, policy_struct=pop.policy_struct)
    env = SimpleNamespace(num_envs=8)
    for make in (lambda: BatchedEvacuationEnv._policy_rollout(None, tf, SimpleNamespace(num_learners=2), 4, None, None, None, None),
                 lambda: BatchedEvacuationEnv._policy_rollout(None, pop.nets[0], views, 4, None, None, None, None),
                 lambda: BatchedEvacuationEnv.policy_evaluate_population(None, tf, 1, 4),
                 lambda: BatchedEvacuationEnv.policy_evaluate_population(None, shaped, 1, 4),
                 lambda: BatchedEvacuationEnv.policy_evaluate_population(None, views, 1, 4),
                 lambda: PopulationEvaluator.evaluate(None, tf),
                 lambda: population.PolicyPopulation(72, [1, 2], "cpu", net=tf),
                 lambda: PopulationTrainer(env, tf, cfg), lambda: PopulationTrainer(env, shaped, cfg),
                 lambda: population.sweep_configs(cfg, {"learning_rate": [1e-3]}, net=tf),
                 lambda: PopulationAdam(SimpleNamespace(num_learners=1, device=CPU, tensors=[], nets=[tf]))):
        with pytest.raises(ValueError, match="attention encoder"):
            make()
    with pytest.raises(ValueError, match="sweeps of transformer learners are not built"):
        BatchedEvacuationEnv.policy_rollout_population(SimpleNamespace(num_envs=8, _is_set_population=BatchedEvacuationEnv._is_set_population,
                                                                       _is_transformer_population=BatchedEvacuationEnv._is_transformer_population),
                                                       pop, 4, None, None, gammas=[0.99, 0.9])
    wet = TransformerPopulation(72, 10, [1, 2], device="cpu")
    for m in wet.nets[0].embedding.modules():
        if isinstance(m, torch.nn.Dropout):
            m.p = 0.1
    with pytest.raises(ValueError, match="dropout p = 0.1"):       # refuse_dropout still applies to collection
        BatchedEvacuationEnv._policy_rollout(None, wet.nets[0], wet, 4, None, None, None, None)
