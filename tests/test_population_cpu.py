"""Population training without a GPU: the new entries are declared, exported and bound; every refusal of
evac_rpo_update_population is decided on the host; the workspace size; the index mapping against a NumPy restatement;
PolicyPopulation's rows against freshly seeded networks; the compiled kernels' resources."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch

from evacuation_amd import _lib, build
from evacuation_amd.policy import LinearActorCritic, _check_structure, mlp_tensors
from tests.kernel_meta import kernel_resources

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INVALID = _lib.ERR_INVALID_ARGUMENT


@pytest.fixture(scope="module")
def lib():
    build.build_library()
    return _lib.load()


def _declaration(name):
    text = open(os.path.join(ROOT, "include", "evac.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    m = re.search(r"\b" + name + r"\s*\(([^;]*)\)\s*;", text)
    assert m, name
    return [a for a in m.group(1).split(",") if a.strip()]


def test_new_symbols_are_declared_exported_and_bound(lib):
    for name, n_args in (("evac_policy_rollout_population", 21), ("evac_rpo_update_population", 30),
                         ("evac_rpo_population_workspace_bytes", 3)):
        assert len(_declaration(name)) == n_args, name
        assert len(_lib.SIGNATURES[name][1]) == n_args, name
        getattr(lib, name)
    # evac_policy_rollout's arguments after (handle, n_learners, policy, strides, n_steps); evac_rpo_update's plus the population's six
    assert len(_declaration("evac_policy_rollout_population")) == len(_declaration("evac_policy_rollout")) + 2
    assert len(_declaration("evac_rpo_update_population")) == len(_declaration("evac_rpo_update")) + 6
    text = open(os.path.join(ROOT, "include", "evac.h")).read()
    assert int(re.search(r"#define EVAC_MAX_LEARNERS (\d+)", text).group(1)) == _lib.MAX_LEARNERS == 64
    assert C.sizeof(_lib.EvacMlpPolicyStrides) == 13 * 8
    assert lib.evac_version() == 150


# ------------------------------------------------------------------------------------------------ refusals, no device
class Call:
    """A well-formed evac_rpo_update_population call on made-up addresses: nothing is dereferenced before the checks."""

    def __init__(self, D=6, S=3, M=64, B_l=256, norm_adv=1):
        H = 64
        self.numel = [H * D, H, H * H, H, 2 * H, 2, 2, H * D, H, H * H, H, H, 1]
        fake = [0x10000 + 0x1000 * i for i in range(13)]
        self.S = S
        self.policy = _lib.EvacMlpPolicy(D, H, *fake)
        self.params, self.grads = _lib.EvacMlpPolicyGrads(*fake), _lib.EvacMlpPolicyGrads(*fake)
        self.pstr, self.gstr, self.mstr = (_lib.EvacMlpPolicyStrides(*self.numel) for _ in range(3))
        self.hstride = 64
        self.loss = _lib.EvacRpoLossConfig(0.2, 0.0, 0.5, 0.5, norm_adv, 1)
        self.adam = _lib.EvacAdamConfig(3e-4, 0.9, 0.999, 1e-5, 0.5)
        self.state = _lib.EvacAdamState(0x20000, _lib.EvacMlpPolicyGrads(*fake), _lib.EvacMlpPolicyGrads(*fake))
        self.B, self.batch = S * B_l, [0x30000 + 0x1000 * i for i in range(6)]
        self.B_l, self.M, self.epochs = B_l, M, 2
        self.perms, self.noise = 0x40000, None
        self.seeds, self.counters = (C.c_uint64 * 64)(*range(64)), (C.c_uint64 * 64)()
        self.stats, self.ws, self.stream = 0x50000, 0x60000, None

    def __call__(self, lib):
        ref = lambda x: None if x is None else C.byref(x)
        return lib.evac_rpo_update_population(
            self.S, ref(self.policy), ref(self.params), ref(self.grads), ref(self.pstr), ref(self.gstr), ref(self.mstr), self.hstride,
            ref(self.loss), ref(self.adam), ref(self.state), self.B, *self.batch, self.B_l, self.M, self.epochs, self.perms, self.noise,
            self.seeds, self.counters, 0, 0.0, self.stats, self.ws, self.stream)


def test_every_refusal_is_decided_on_the_host(lib):
    def refused(**kw):
        c = Call(**{k: kw.pop(k) for k in ("D", "S", "M", "B_l", "norm_adv") if k in kw})
        for k, v in kw.items():
            if callable(v):
                v(c)
            else:
                setattr(c, k, v)
        return c(lib)

    for S in (0, -1, 65):
        assert refused(S=S) == INVALID, S
    for field in ("policy", "params", "grads", "pstr", "gstr", "mstr", "loss", "adam", "state", "perms", "seeds", "counters", "stats", "ws"):
        assert refused(**{field: None}) == INVALID, field
    for k in range(6):                                            # each batch array NULL in turn
        assert refused(batch=lambda c, k=k: c.batch.__setitem__(k, None)) == INVALID, k
    for struct in ("policy", "params", "grads"):                  # a NULL tensor
        assert refused(**{struct + "_": lambda c, s=struct: setattr(getattr(c, s), "critic_b2", None)}) == INVALID, struct
    assert refused(header_=lambda c: setattr(c.state, "header", None)) == INVALID
    assert refused(moment_=lambda c: setattr(c.state.exp_avg_sq, "actor_w1", None)) == INVALID
    for which in ("pstr", "gstr", "mstr"):                        # a stride of 0 (or smaller than its tensor) with S > 1
        assert refused(**{which + "_": lambda c, w=which: setattr(getattr(c, w), "actor_w2", 0)}) == INVALID, which
        assert refused(**{which + "_": lambda c, w=which: setattr(getattr(c, w), "critic_b3", 0)}) == INVALID, which
        assert refused(**{which + "_": lambda c, w=which: setattr(getattr(c, w), "actor_w1", 64 * 6 - 1)}) == INVALID, which
    for hstride in (0, 32, 60, 68, 100):                          # the header stride: >= 64 and a multiple of 8
        assert refused(hstride=hstride) == INVALID, hstride
    assert refused(ws=0x60008) == INVALID                          # the workspace: 16-byte aligned
    assert refused(header_=lambda c: setattr(c.state, "header", 0x20004)) == INVALID
    for D in (0, -3, 397):
        assert refused(D=D) == INVALID, D
    assert refused(M=1, norm_adv=1) == INVALID                     # B_l < 2 with norm_adv: the unbiased std of one sample
    assert refused(M=1, B_l=1, norm_adv=1) == INVALID
    assert refused(B_l=0) == INVALID and refused(M=0) == INVALID and refused(epochs=0) == INVALID and refused(B=0) == INVALID
    assert refused(hidden_=lambda c: setattr(c.policy, "hidden", 32)) == INVALID
    assert refused(lr_=lambda c: setattr(c.adam, "lr", float("nan"))) == INVALID
    # the rollout entry needs a handle: without one it is refused before anything else
    assert lib.evac_policy_rollout_population(None, 3, None, None, 4, *([None] * 11), 0.99, 1.0, 100.0, 1e-8, None) == INVALID


def test_workspace_is_one_aligned_slice_per_learner(lib):
    for D, M in ((6, 192), (6, 2), (124, 1000), (396, 16384), (17, 333)):
        one = lib.evac_rpo_workspace_bytes(D, M)
        slice_ = (one + 127) // 128 * 128                          # a learner's slice starts on a 128-byte line of its own
        for S in (1, 2, 10, 64):
            assert lib.evac_rpo_population_workspace_bytes(D, M, S) == S * slice_, (D, M, S)
            assert S * one <= S * slice_ < S * (one + 128)
    for bad in ((0, 64, 2), (397, 64, 2), (6, 0, 2), (6, 64, 0), (6, 64, 65)):
        assert lib.evac_rpo_population_workspace_bytes(*bad) == INVALID, bad


# ------------------------------------------------------------------------------------------------ the Python face
@pytest.mark.parametrize("E_l", [1, 3, 16, 48])
def test_index_mapping_against_numpy(E_l):
    from evacuation_amd.population import population_rows
    S, T = 5, 7
    B_l = T * E_l
    common = np.arange(T * S * E_l).reshape(T, S, E_l)             # the common batch's rows, time-major over the whole env
    rng = np.random.default_rng(E_l)
    perms = np.stack([np.stack([rng.permutation(B_l) for _ in range(3)]) for _ in range(S)])        # [S, epochs, B_l]
    got = population_rows(torch.from_numpy(perms), torch.arange(S).reshape(S, 1, 1), E_l, S).numpy()
    for s in range(S):
        own = common[:, s, :].reshape(-1)                          # learner s's batch, flattened as a trainer of E_l envs flattens it
        assert np.array_equal(got[s], own[perms[s]]), (E_l, s)
        assert np.array_equal(population_rows(torch.from_numpy(perms[s]), s, E_l, S).numpy(), own[perms[s]])
        assert sorted(got[s, 0].tolist()) == sorted(own.tolist())  # every row of the learner, once per epoch, nobody else's
    assert got.dtype == np.int64 and got.min() == 0 and got.max() == T * S * E_l - 1


@pytest.mark.parametrize("D", [6, 124])
def test_population_rows_are_freshly_seeded_networks(D):
    from evacuation_amd.population import PolicyPopulation
    seeds = [5, 1, 20261017]
    torch.manual_seed(99)
    before = torch.rand(3)
    torch.manual_seed(99)
    pop = PolicyPopulation(D, seeds, device="cpu")
    assert torch.equal(torch.rand(3), before)                       # the caller's generator is where it was
    assert pop.num_learners == 3 and len(pop.tensors) == 13
    for s, seed in enumerate(seeds):
        torch.manual_seed(seed)
        fresh = LinearActorCritic(D)
        _check_structure(pop.nets[s], D, torch.device("cpu"))
        for i, (a, b) in enumerate(zip(mlp_tensors(pop.nets[s]), mlp_tensors(fresh))):
            assert a.shape == b.shape and torch.equal(a.detach().view(torch.int32), b.detach().view(torch.int32)), (s, i)
            assert a.data_ptr() == pop.tensors[i][s].data_ptr() and a.is_contiguous()       # a view of row s
            assert a.grad is not None and a.grad.data_ptr() == pop.grads[i][s].data_ptr()
        assert len(list(pop.nets[s].parameters())) == 13
    strides = [getattr(pop.strides, f) for f, _ in _lib.EvacMlpPolicyStrides._fields_]
    assert strides == [t[0].numel() for t in pop.tensors]
    with torch.no_grad():                                           # an in-place update of the stack is the nets' update
        pop.tensors[2][1].add_(1.0)
    assert torch.equal(pop.nets[1].actor_mean[2].weight.detach(), pop.tensors[2][1])
    with pytest.raises(ValueError):
        PolicyPopulation(D, [], device="cpu")
    with pytest.raises(ValueError):
        PolicyPopulation(D, list(range(65)), device="cpu")


# ------------------------------------------------------------------------------------------------ the compiled kernels
def test_population_update_kernels_use_no_scratch_and_keep_the_register_class():
    pop = kernel_resources("evac_population_api.hip")
    one = kernel_resources("evac_train_api.hip")
    assert len(pop) == 5, list(pop)
    assert not any(t in n for n in pop for t in ("k_rollout", "k_step", "k_policy_evaluate", "k_gae", "k_adam", "k_rpo"))
    for name, k in pop.items():
        assert k["private_segment_fixed_size"] == 0 and k["vgpr_spill_count"] == 0, (name, k)

    def vgprs(kernels, stem):
        found = [k["vgpr_count"] for n, k in kernels.items() if stem in n]
        assert found, stem
        return max(found)

    def waves_per_simd(v):                                          # 512 VGPRs per SIMD lane, allocated in blocks of 8
        return min(8, 512 // ((v + 7) // 8 * 8))
    for mine, theirs in (("k_population_adv_stats", "k_rpo_adv_stats"), ("k_population_grad", "k_rpo_grad"),
                         ("k_population_finish", "k_rpo_finish"), ("k_population_optimizer", "k_adam")):
        assert waves_per_simd(vgprs(pop, mine)) >= waves_per_simd(vgprs(one, theirs)), (mine, vgprs(pop, mine), vgprs(one, theirs))
    assert vgprs(pop, "k_population_grad") <= vgprs(one, "k_rpo_grad")
    assert len(one) == 8                                            # evac_train_api.hip's own kernels are as they were


def test_population_collection_kernels_fit_the_register_budget():
    kernels = kernel_resources("evac_api.hip")
    mine = {n: k for n, k in kernels.items() if "k_collect_population" in n}
    assert len(mine) == 8, list(mine)                               # gravity / generic observation x chain on / off x default config or not
    for name, k in mine.items():
        assert k["vgpr_count"] <= 128 and k["vgpr_spill_count"] == 0 and k["private_segment_fixed_size"] == 0, (name, k)
        assert not any(t in name for t in ("k_rollout", "k_step", "k_policy_evaluate", "k_gae", "k_adam", "k_rpo"))
    assert sum("k_policy_rollout<" in n for n in kernels) == 8 and sum("k_policy_evaluate" in n for n in kernels) == 10
