"""CPU tests of the population of deep-sets leaders (include/evac.h: evac_deepsets_strides_t, evac_policy_rollout_population_deepsets,
evac_deepsets_population_workspace_bytes, evac_deepsets_update_population; evacuation_amd.population.DeepSetsPopulation): the
symbols, every refusal with no device present (no pointer is ever followed: they are made-up addresses), the workspace's size,
the Python face on the CPU and the compiled kernels of the new translation unit."""
import ctypes as C
import os
import re
from types import SimpleNamespace

import pytest
import torch

from evacuation_amd import _lib, build
from evacuation_amd.policy import DeepSetsActorCritic, TransformerActorCritic, _check_encoder, _check_structure, all_tensors
from tests.kernel_meta import kernel_resources

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BAD = _lib.ERR_INVALID_ARGUMENT
FAKE = 0x1000                                    # 16-byte aligned, never followed
UNIT = "evac_deepsets_population_api.hip"


@pytest.fixture(scope="module")
def lib():
    build.build_library()
    return _lib.load()


def test_symbols_are_declared_exported_and_bound(lib):
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "evac.h")).read(), flags=re.S)
    counts = {}
    for name in ("evac_policy_rollout_population_deepsets", "evac_policy_rollout_population", "evac_deepsets_update_population",
                 "evac_rpo_update_population"):
        decl = re.search(rf"int {name}\((.*?)\);", text, re.S)
        assert decl and name in _lib.SIGNATURES, name
        fn = getattr(lib, name)
        counts[name] = len(decl.group(1).split(","))
        assert len(fn.argtypes) == counts[name] and fn.restype is C.c_int, name
    assert counts["evac_policy_rollout_population_deepsets"] == counts["evac_policy_rollout_population"] + 2 == 23     # encoder, strides
    # the encoder, its parameters and gradients, and a strides struct beside each of the three
    assert counts["evac_deepsets_update_population"] == counts["evac_rpo_update_population"] + 6 == 36
    assert re.search(r"int64_t evac_deepsets_population_workspace_bytes\(int32_t \w+, int64_t \w+, int32_t \w+\);", text)
    sizer = lib.evac_deepsets_population_workspace_bytes
    assert sizer.restype is C.c_int64 and len(sizer.argtypes) == 3
    body = re.search(r"typedef struct evac_deepsets_strides \{(.*?)\} evac_deepsets_strides_t;", text, re.S).group(1)
    assert re.findall(r"(\w+)[,;]", body) == [f for f, _ in _lib.EvacDeepSetsStrides._fields_] and "int64_t" in body
    assert [f for f, _ in _lib.EvacDeepSetsStrides._fields_] == [f for f, _ in _lib.EvacDeepSets._fields_[2:]]
    assert C.sizeof(_lib.EvacDeepSetsStrides) == 6 * 8
    assert lib.evac_version() == _lib.VERSION == 150
    unit = os.path.join(build.CSRC, UNIT)
    assert unit in build.SOURCES and build.SOURCES[-1] != unit


# ------------------------------------------------------------------------------------------------ refusals
def enc_sizes(D, ed):
    return [24 * ed, 24, 24 * 24, 24, D * 24, D]


def mlp_sizes(D):
    return [64 * D, 64, 64 * 64, 64, 128, 2, 2, 64 * D, 64, 64 * 64, 64, 64, 1]


class Update:
    """A call of evac_deepsets_update_population whose every argument is acceptable, to be spoiled one argument at a time."""

    def __init__(self, S=2, D=36, ed=3, M=4, B_l=8, norm_adv=1, epochs=2):
        self.S, self.D, self.ed, self.M, self.B_l, self.epochs = S, D, ed, M, B_l, epochs
        self.pol = _lib.EvacMlpPolicy(D, 64, *[FAKE] * 13)
        self.enc = _lib.EvacDeepSets(ed, 24, *[FAKE] * 6)
        self.params, self.grads = _lib.EvacMlpPolicyGrads(*[FAKE] * 13), _lib.EvacMlpPolicyGrads(*[FAKE] * 13)
        self.enc_params, self.enc_grads = _lib.EvacDeepSetsGrads(*[FAKE] * 6), _lib.EvacDeepSetsGrads(*[FAKE] * 6)
        self.strides = [_lib.EvacMlpPolicyStrides(*mlp_sizes(D)) for _ in range(3)]
        self.enc_strides = [_lib.EvacDeepSetsStrides(*enc_sizes(D, ed)) for _ in range(3)]
        self.header_stride = 64
        self.cfg = _lib.EvacRpoLossConfig(0.2, 0.0, 0.5, 0.5, norm_adv, 1)
        self.adam = _lib.EvacAdamConfig(3e-4, 0.9, 0.999, 1e-5, 0.5)
        self.state = _lib.EvacDeepSetsAdamState(FAKE, _lib.EvacMlpPolicyGrads(*[FAKE] * 13), _lib.EvacMlpPolicyGrads(*[FAKE] * 13),
                                                _lib.EvacDeepSetsGrads(*[FAKE] * 6), _lib.EvacDeepSetsGrads(*[FAKE] * 6))
        self.null = set()                        # names of struct arguments passed as NULL
        self.seeds = self.counters = True
        self.workspace = FAKE
        self.batch = S * B_l

    def ref(self, name, obj):
        return None if name in self.null else C.byref(obj)

    def __call__(self, lib):
        u64 = (C.c_uint64 * max(self.S, 1))()
        r = self.ref
        return lib.evac_deepsets_update_population(
            self.S, r("pol", self.pol), r("enc", self.enc), r("params", self.params), r("enc_params", self.enc_params),
            r("grads", self.grads), r("enc_grads", self.enc_grads), r("param_strides", self.strides[0]),
            r("enc_param_strides", self.enc_strides[0]), r("grad_strides", self.strides[1]), r("enc_grad_strides", self.enc_strides[1]),
            r("moment_strides", self.strides[2]), r("enc_moment_strides", self.enc_strides[2]), self.header_stride, r("cfg", self.cfg),
            r("adam", self.adam), r("state", self.state), self.batch, *[FAKE] * 6, self.B_l, self.M, self.epochs, FAKE, None,
            u64 if self.seeds else None, u64 if self.counters else None, 1, 0.01, FAKE, self.workspace, None)


def test_update_refusals_without_a_device(lib):
    """Every refusal is decided on the host: the pointers are made up, and a call that got past the checks would follow them."""
    def refused(call, why):
        assert call(lib) == BAD, why

    for S in (0, 65):
        refused(Update(S=S), f"n_learners {S}")
    for name in ("param_strides", "enc_param_strides", "grad_strides", "enc_grad_strides", "moment_strides", "enc_moment_strides",
                 "pol", "enc", "params", "enc_params", "grads", "enc_grads", "cfg", "adam", "state"):
        call = Update()
        call.null.add(name)
        refused(call, f"NULL {name}")
    for which in range(3):                       # parameters, gradients, moments
        for field, least in zip([f for f, _ in _lib.EvacDeepSetsStrides._fields_], enc_sizes(36, 3)):
            for value in (least - 1, 0):
                call = Update()
                setattr(call.enc_strides[which], field, value)
                refused(call, f"encoder stride {which}.{field} = {value} with S = 2")
        call = Update()
        call.enc_strides[which].rho_w = 36 * 24 + 2          # 16-byte alignment of learner 1's rho_w
        refused(call, f"rho_w stride {which} not a multiple of 4")
        call = Update()
        call.strides[which].actor_w1 = 64 * 36 - 1
        refused(call, f"policy stride {which} below its tensor")
    for stride in (56, 68):
        call = Update()
        call.header_stride = stride
        refused(call, f"header stride {stride}")
    call = Update()
    call.workspace = FAKE + 8
    refused(call, "a misaligned workspace")
    refused(Update(epochs=0), "n_epochs 0")
    refused(Update(B_l=0), "learner_batch_size 0")
    refused(Update(ed=7, D=42), "set_elem_dim 7")
    refused(Update(ed=5, D=36), "D not a multiple of set_elem_dim")
    refused(Update(M=1), "one sample with norm_adv")
    for flag in ("seeds", "counters"):
        call = Update()
        setattr(call, flag, False)
        refused(call, f"NULL {flag}")
    # S = 1: the strides are not held against the tensors (nobody is s x stride further): the call gets to the NEXT check, the
    # optimiser's tensors, which refuses a NULL moment -- so nothing is followed
    call = Update(S=1)
    for which in range(3):
        for field in [f for f, _ in _lib.EvacDeepSetsStrides._fields_]:
            setattr(call.enc_strides[which], field, 0)
        call.enc_strides[which].rho_w = 2
    call.header_stride = 0
    call.state.enc_exp_avg_sq.rho_b = None
    refused(call, "S = 1 with zero strides, up to the optimiser's NULL moment")
    call = Update(S=1)
    call.null.add("enc_moment_strides")          # a NULL strides struct is refused at S = 1 too
    refused(call, "S = 1 with a NULL strides struct")


def test_collection_refuses_without_a_handle(lib):
    """Without a handle the collection entry is refused before anything else, whatever its other arguments: that alone is shown
    here.  Its own refusals -- the strides, the learners' number and shares -- need a handle, which needs a device: their table
    of codes and texts is tests/test_gpu_deepsets_population.py::test_collection_entry_refusals_have_their_code_and_text_and_enqueue_nothing."""
    pol, enc = _lib.EvacMlpPolicy(36, 64, *[FAKE] * 13), _lib.EvacDeepSets(3, 24, *[FAKE] * 6)
    st, est = _lib.EvacMlpPolicyStrides(*mlp_sizes(36)), _lib.EvacDeepSetsStrides(*enc_sizes(36, 3))
    p = C.c_void_p(FAKE)
    for strides, enc_strides in ((C.byref(st), C.byref(est)), (None, C.byref(est)), (C.byref(st), None)):
        rc = lib.evac_policy_rollout_population_deepsets(None, 2, C.byref(pol), strides, C.byref(enc), enc_strides, 4, *[p] * 11,
                                                         0.99, 10.0, 10.0, 1e-8, None)
        assert rc == BAD


def test_workspace_bytes(lib):
    pop, one = lib.evac_deepsets_population_workspace_bytes, lib.evac_deepsets_workspace_bytes
    for D, M in ((6, 8), (36, 72), (372, 192), (396, 1024)):
        lone = one(D, M)
        assert lone > 0
        last = 0
        for S in (1, 2, 3, 8, 64):
            need = pop(D, M, S)
            assert need >= S * lone and need > last, (D, M, S, need, lone)
            # the slices, and the learners' encoded batch and gathered columns once more as one common batch (256-byte parts)
            assert need <= S * (lone + 256 + 4 * M * (D + 6) + 8 * M) + 8 * 256, (D, M, S, need, lone)
            last = need
    for bad in ((0, 64, 2), (397, 64, 2), (6, 0, 2), (6, 64, 0), (6, 64, 65)):
        assert pop(*bad) == BAD, bad
        if bad[2] == 2:
            assert one(*bad[:2]) == BAD, bad


# ------------------------------------------------------------------------------------------------ the Python face
def test_population_rows_are_freshly_seeded_networks():
    from evacuation_amd.population import DeepSetsPopulation
    D, N, seeds = 36, 10, [5, 1, 20261017]
    torch.manual_seed(99)
    before = torch.rand(3)
    torch.manual_seed(99)
    pop = DeepSetsPopulation(D, N, seeds, device="cpu")
    assert torch.equal(torch.rand(3), before)                       # the caller's generator is where it was
    assert pop.num_learners == 3 and len(pop.tensors) == 19 and len(pop.grads) == 19 and pop.set_elem_dim == 3
    shapes = [(64, D), (64,), (64, 64), (64,), (2, 64), (2,), (1, 2), (64, D), (64,), (64, 64), (64,), (1, 64), (1,),
              (24, 3), (24,), (24, 24), (24,), (D, 24), (D,)]
    assert [tuple(t.shape) for t in pop.tensors] == [(3,) + s for s in shapes]
    assert not hasattr(pop, "deep_sets") and not hasattr(pop, "embedding")       # (refuse_deepsets would take it for a network)
    for s, seed in enumerate(seeds):
        torch.manual_seed(seed)
        fresh = DeepSetsActorCritic(D, N)
        _check_structure(pop.nets[s], D, torch.device("cpu"))
        assert _check_encoder(pop.nets[s], D, torch.device("cpu"), N) == 3
        for i, (a, b) in enumerate(zip(all_tensors(pop.nets[s]), all_tensors(fresh))):
            assert a.shape == b.shape and torch.equal(a.detach().view(torch.int32), b.detach().view(torch.int32)), (s, i)
            assert a.data_ptr() == pop.tensors[i][s].data_ptr() and a.is_contiguous()       # a view of row s
            assert a.grad is not None and a.grad.data_ptr() == pop.grads[i][s].data_ptr()
        assert len(list(pop.nets[s].parameters())) == 19
    assert [getattr(pop.strides, f) for f, _ in _lib.EvacMlpPolicyStrides._fields_] == [t[0].numel() for t in pop.tensors[:13]]
    assert [getattr(pop.encoder_strides, f) for f, _ in _lib.EvacDeepSetsStrides._fields_] == [t[0].numel() for t in pop.tensors[13:]]
    assert pop.encoder_strides.rho_w % 4 == 0
    assert pop.policy_struct().actor_w1 == pop.tensors[0].data_ptr() and pop.encoder_struct().rho_w == pop.tensors[17].data_ptr()
    with torch.no_grad():                                           # an in-place update of the stack is the nets' update
        pop.tensors[15][1].add_(1.0)
    assert torch.equal(pop.nets[1].deep_sets.transform_phi[2].weight.detach(), pop.tensors[15][1])
    x = torch.randn(4, D)
    with torch.no_grad():                                           # the views compute what the module computes
        assert pop.nets[2].get_value(x).shape == (4, 1)
    with pytest.raises(ValueError, match="0 learners"):
        DeepSetsPopulation(D, N, [], device="cpu")
    with pytest.raises(ValueError, match="65 learners"):
        DeepSetsPopulation(D, N, list(range(65)), device="cpu")
    with pytest.raises(ValueError, match="whole number"):
        DeepSetsPopulation(37, N, [1], device="cpu")


def test_the_pinned_refusals_keep_their_message():
    from evacuation_amd.population import DeepSetsPopulation, PolicyPopulation, PopulationTrainer, sweep_configs
    from evacuation_amd.trainer import RPOTrainingConfig
    net = DeepSetsActorCritic(36, 10)
    cfg = RPOTrainingConfig(num_envs=4, num_steps=8, num_minibatches=2)
    env = SimpleNamespace(num_envs=4)
    says = "gradient and optimiser kernels are the linear network's"
    with pytest.raises(ValueError, match=says):
        PolicyPopulation(36, [1, 2], device="cpu", net=net)
    with pytest.raises(ValueError, match=says):
        PopulationTrainer(env, net, cfg)
    with pytest.raises(ValueError, match=says):
        sweep_configs(cfg, {"learning_rate": [1e-3, 3e-4]}, net=net)
    tf = TransformerActorCritic(36, 10)
    for make in (lambda: PolicyPopulation(36, [1, 2], device="cpu", net=tf), lambda: PopulationTrainer(env, tf, cfg),
                 lambda: sweep_configs(cfg, {"learning_rate": [1e-3]}, net=tf)):
        with pytest.raises(ValueError, match="attention encoder"):
            make()
    # a list of differing configurations, and an env the learners do not divide, are refused before any device is needed
    import dataclasses
    pop = DeepSetsPopulation(36, 10, [1, 2], device="cpu")
    with pytest.raises(ValueError, match="sweeps of deep-sets learners are not built"):
        PopulationTrainer(SimpleNamespace(num_envs=8), pop, [cfg, dataclasses.replace(cfg, learning_rate=1e-3)])
    with pytest.raises(ValueError, match="1 configurations for 2 learners"):
        PopulationTrainer(SimpleNamespace(num_envs=8), pop, [cfg])
    with pytest.raises(ValueError, match="2 learners x cfg.num_envs"):
        PopulationTrainer(SimpleNamespace(num_envs=9), pop, cfg)


# ------------------------------------------------------------------------------------------------ the compiled kernels
def _vgprs(kernels, stem):
    found = [k["vgpr_count"] for n, k in kernels.items() if stem in n]
    assert found, stem
    return max(found)


def _waves_per_simd(v):                                             # 512 VGPRs per SIMD lane, allocated in blocks of 8
    return min(8, 512 // ((v + 7) // 8 * 8))


def test_the_new_unit_holds_the_kernels_design_names_with_no_scratch():
    mine = kernel_resources(UNIT)
    lone = kernel_resources("evac_deepsets_update_api.hip")
    stems = sorted(n.split("(")[0].replace("void ", "") for n in mine)
    gate = "<evac::AdamHeader const*, evac::SetLearnerStrides>"
    assert stems == sorted(["evac::k_adam_set_population", "evac::k_set_encode" + gate, "evac::k_set_backward" + gate,
                            "evac::k_set_finish" + gate] +
                           [f"evac::k_collect_population_deepsets<{n}, {d}>" for n in ("true", "false") for d in ("true", "false")]), stems
    design = open(os.path.join(ROOT, "DESIGN.md")).read()
    assert "evac_deepsets_population_api.hip: 8 kernels" in design
    for stem in ("k_collect_population_deepsets", "k_adam_set_population", "k_set_encode", "k_set_backward", "k_set_finish"):
        assert stem in design
    # no actor-critic kernel is defined a second time: the middle of a step is evac_population_api.hip's
    assert not any(t in n for n in mine for t in ("k_rpo", "k_population", "k_gae", "k_policy_rollout", "k_policy_evaluate", "k_adam_set("))
    for name, k in mine.items():
        assert k["private_segment_fixed_size"] == 0 and k["vgpr_spill_count"] == 0, (name, k)
        if "k_collect_population_deepsets" in name:
            assert k["vgpr_count"] <= 128, (name, k)
    # waves per SIMD not below the gated lone twin's
    for sibling, twin in (("k_set_encode", "k_set_encode<evac::AdamHeader const*>"), ("k_set_backward", "k_set_backward<evac::AdamHeader const*>"),
                          ("k_set_finish", "k_set_finish<evac::AdamHeader const*>"), ("k_adam_set_population", "k_adam_set")):
        assert _waves_per_simd(_vgprs(mine, sibling)) >= _waves_per_simd(_vgprs(lone, twin)), (sibling, _vgprs(mine, sibling), _vgprs(lone, twin))
    assert len(lone) == 13                                          # evac_deepsets_update_api.hip's own kernels are as they were
