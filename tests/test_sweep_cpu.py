"""Population sweeps without a GPU: the three new entries are declared, exported and bound; every refusal of the learners'
values is decided on the host, for a learner that is not learner 0; sweep_configs; the structural check of PopulationTrainer;
PopulationAdam's per-learner param groups; the compiled kernels' resources and names."""
import ctypes as C
import os
import re

import pytest
import torch

from evacuation_amd import _lib, build
from evacuation_amd.trainer import RPOTrainingConfig
from tests.kernel_meta import kernel_resources
from tests.test_population_cpu import Call, _declaration

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INVALID = _lib.ERR_INVALID_ARGUMENT
NAN, INF = float("nan"), float("inf")


@pytest.fixture(scope="module")
def lib():
    build.build_library()
    return _lib.load()


def test_new_symbols_are_declared_exported_and_bound(lib):
    for name, n_args in (("evac_gae_learners", 13), ("evac_policy_rollout_sweep", 22), ("evac_rpo_update_sweep", 29)):
        assert len(_declaration(name)) == n_args, name
        assert len(_lib.SIGNATURES[name][1]) == n_args, name
        getattr(lib, name)
    # evac_gae's arguments plus (envs_per_learner, n_learners, hypers) in place of (gamma, gae_lambda); the population's rollout
    # plus hypers; the population's update with hypers in place of (use_target_kl, target_kl)
    assert len(_declaration("evac_gae_learners")) == len(_declaration("evac_gae")) + 1
    assert len(_declaration("evac_policy_rollout_sweep")) == len(_declaration("evac_policy_rollout_population")) + 1
    assert len(_declaration("evac_rpo_update_sweep")) == len(_declaration("evac_rpo_update_population")) - 1
    text = open(os.path.join(ROOT, "include", "evac.h")).read()
    body = re.search(r"typedef struct evac_learner_hyper \{(.*?)\} evac_learner_hyper_t;", text, flags=re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    size = {"double": 8, "float": 4, "int32_t": 4}
    fields = []
    for decl in body.split(";"):
        if decl.strip():
            kind, names = decl.split(None, 1)
            fields += [(n.strip(), kind) for n in names.split(",")]
    assert [f for f, _ in fields] == [f for f, _ in _lib.EvacLearnerHyper._fields_]
    assert sum(size[k] for _, k in fields) == C.sizeof(_lib.EvacLearnerHyper) == 56      # (no padding: doubles first)
    assert lib.evac_version() == 150


# ------------------------------------------------------------------------------------------------ refusals, no device
class SweepCall(Call):
    """A well-formed evac_rpo_update_sweep call on made-up addresses (tests/test_population_cpu.Call with the learners' values)."""

    def __init__(self, **kw):
        super().__init__(**kw)
        n = max(1, min(self.S, 64))
        self.hypers = _lib.learner_hypers(n, learning_rate=[1e-4 * (s + 1) for s in range(n)], target_kl=0.02)

    def __call__(self, lib):
        ref = lambda x: None if x is None else C.byref(x)
        return lib.evac_rpo_update_sweep(
            self.S, ref(self.policy), ref(self.params), ref(self.grads), ref(self.pstr), ref(self.gstr), ref(self.mstr), self.hstride,
            ref(self.loss), ref(self.adam), ref(self.state), self.B, *self.batch, self.B_l, self.M, self.epochs, self.perms, self.noise,
            self.seeds, self.counters, self.hypers, self.stats, self.ws, self.stream)


BAD_VALUES = [("learning_rate", NAN), ("learning_rate", INF), ("learning_rate", -INF), ("max_grad_norm", 0.0), ("max_grad_norm", -1.0),
              ("max_grad_norm", NAN), ("clip_coef", -0.1), ("clip_coef", NAN), ("rpo_alpha", -0.5), ("rpo_alpha", NAN), ("gamma", NAN),
              ("gamma", INF), ("gae_lambda", NAN), ("gae_lambda", -INF), ("target_kl", NAN)]


def test_every_refusal_of_the_update_is_decided_on_the_host(lib):
    def refused(**kw):
        c = SweepCall(**{k: kw.pop(k) for k in ("D", "S", "M", "B_l", "norm_adv") if k in kw})
        for k, v in kw.items():
            if callable(v):
                v(c)
            else:
                setattr(c, k, v)
        return c(lib)

    assert refused(hypers=None) == INVALID
    for learner in (1, 2):                                         # never learner 0: every entry of the array is read
        for field, bad in BAD_VALUES:
            assert refused(bad_=lambda c: setattr(c.hypers[learner], field, bad)) == INVALID, (learner, field, bad)
    # a NaN target of a learner WITHOUT a target is not looked at: the call gets past the hypers (and is refused for its workspace)
    def nan_unused(c):
        c.hypers[1].use_target_kl = 0
        c.hypers[1].target_kl = NAN
        c.ws = 0x60008
    assert refused(ok_=nan_unused) == INVALID
    # what the population entry refuses already
    for S in (0, -1, 65):
        assert refused(S=S) == INVALID, S
    for field in ("policy", "params", "grads", "pstr", "gstr", "mstr", "loss", "adam", "state", "perms", "seeds", "counters", "stats", "ws"):
        assert refused(**{field: None}) == INVALID, field
    for hstride in (0, 32, 60, 68):
        assert refused(hstride=hstride) == INVALID, hstride
    assert refused(ws=0x60008) == INVALID and refused(D=397) == INVALID and refused(M=1, norm_adv=1) == INVALID
    assert refused(epochs=0) == INVALID and refused(B_l=0) == INVALID
    assert refused(pstr_=lambda c: setattr(c.pstr, "actor_w2", 0)) == INVALID


def test_every_refusal_of_gae_and_rollout_is_decided_on_the_host(lib):
    fake = [0x10000 + 0x1000 * i for i in range(7)]

    def gae(S=3, E_l=5, E=None, T=4, hypers="ok", null=None, edit=None):
        h = _lib.learner_hypers(S if 1 <= S <= 64 else 1, target_kl=0.02) if hypers == "ok" else hypers
        if edit:
            edit(h)
        a = list(fake)
        if null is not None:
            a[null] = None
        return lib.evac_gae_learners(T, S * E_l if E is None else E, *a[:5], E_l, S, h, a[5], a[6], None)

    assert gae(hypers=None) == INVALID
    for field, bad in BAD_VALUES:
        assert gae(edit=lambda h: setattr(h[2], field, bad)) == INVALID, (field, bad)
    for k in range(7):
        assert gae(null=k) == INVALID, k
    assert gae(T=0) == INVALID and gae(S=0) == INVALID and gae(S=65) == INVALID and gae(E_l=0) == INVALID
    assert gae(E=14) == INVALID and gae(E=16) == INVALID and gae(E=10) == INVALID        # E != S E_l
    # the rollout entry needs a handle: without one it is refused before anything else
    assert lib.evac_policy_rollout_sweep(None, 3, None, None, 4, *([None] * 11), 0.99, 1.0, 100.0, 1e-8, _lib.learner_hypers(3), None) == INVALID


def test_learner_hypers_columns():
    h = _lib.learner_hypers(3, learning_rate=[1e-4, 2e-4, 3e-4], gamma=0.9, target_kl=[None, 0.0, 0.5], max_grad_norm=(0.1, 0.2, 0.3))
    assert [x.learning_rate for x in h] == [1e-4, 2e-4, 3e-4] and [x.gamma for x in h] == [0.9] * 3
    assert [x.use_target_kl for x in h] == [0, 1, 1] and [x.target_kl for x in h] == [0.0, 0.0, 0.5]
    assert [x.max_grad_norm for x in h] == [C.c_float(v).value for v in (0.1, 0.2, 0.3)]
    assert h[0].gae_lambda == 0.95 and h[0].clip_coef == C.c_float(0.2).value and h[0].vf_coef == 0.5 and h[0].rpo_alpha == 0.5
    with pytest.raises(ValueError):
        _lib.learner_hypers(3, gamma=[0.9, 0.99])
    with pytest.raises(ValueError):
        _lib.learner_hypers(3, num_minibatches=4)
    with pytest.raises(ValueError):
        _lib.learner_hypers(65)


# ------------------------------------------------------------------------------------------------ the Python face
def test_sweep_configs_product_order_and_cap():
    from evacuation_amd.population import MAX_LEARNERS, sweep_configs
    base = RPOTrainingConfig(seed=7, num_envs=3, num_steps=64, gamma=0.97)
    got = sweep_configs(base, {"learning_rate": [1e-4, 3e-4, 1e-3], "ent_coef": [0.0, 0.01]}, seeds=[1, 2])
    assert len(got) == 12
    want = [(lr, ent, seed) for lr in (1e-4, 3e-4, 1e-3) for ent in (0.0, 0.01) for seed in (1, 2)]       # the seeds vary fastest
    assert [(c.learning_rate, c.ent_coef, seed) for seed, c in got] == want
    assert all(c.seed == seed and c.gamma == 0.97 and c.num_steps == 64 for seed, c in got)
    assert base.learning_rate == 3e-4 and base.seed == 7           # the base is not touched
    assert [(s, c.seed, c.learning_rate) for s, c in sweep_configs(base, {})] == [(7, 7, 3e-4)]
    assert len(sweep_configs(base, {"gamma": [0.9] * 8}, seeds=range(8))) == 64 == MAX_LEARNERS
    with pytest.raises(ValueError, match="65"):
        sweep_configs(base, {"gamma": [0.9] * 13}, seeds=range(5))
    with pytest.raises(ValueError, match="lerning_rate"):
        sweep_configs(base, {"lerning_rate": [1.0]})
    with pytest.raises(ValueError):
        sweep_configs(base, {"gamma": []})


class _FakeEnv:
    def __init__(self, n):
        self.num_envs = n


def _cpu_population(S, D=6):
    from evacuation_amd.population import PolicyPopulation
    return PolicyPopulation(D, list(range(1, S + 1)), device="cpu")


def test_population_adam_has_one_param_group_per_learner(monkeypatch):
    from evacuation_amd import population, trainer
    monkeypatch.setattr(trainer.DeviceAdam, "__init__", _host_adam_init)
    pop = _cpu_population(3)
    opt = population.PopulationAdam(pop, lr=[1e-4, 2e-4, 3e-4], max_grad_norm=0.5)
    assert [g["lr"] for g in opt.param_groups] == [1e-4, 2e-4, 3e-4] and not opt.uniform()
    opt.learners[1].param_groups[0]["lr"] = 7.0
    assert opt.learners[0].param_groups[0]["lr"] == 1e-4 and opt.learners[2].param_groups[0]["lr"] == 3e-4
    assert [g["lr"] for g in opt.param_groups] == [1e-4, 7.0, 3e-4]
    assert opt.learners[0].param_groups is not opt.learners[1].param_groups
    assert opt.config(1).lr == 7.0 and opt.config(0).lr == 1e-4 and opt.config().lr == 1e-4
    opt.set_lr(5e-4)
    assert opt.uniform() and [g["lr"] for g in opt.param_groups] == [5e-4] * 3
    one = population.PopulationAdam(pop, lr=1e-3)
    assert one.uniform() and [g["lr"] for g in one.param_groups] == [1e-3] * 3
    one.learners[2].param_groups[0]["eps"] = 1e-3                   # eps is one value for all: a learner's own is an error
    with pytest.raises(ValueError, match="learner 2"):
        one.config()
    with pytest.raises(ValueError):
        population.PopulationAdam(pop, lr=[1e-4, 2e-4])


def _host_adam_init(self, net, lr=3e-4, betas=(0.9, 0.999), eps=1e-5, max_grad_norm=0.5, *, storage=None):
    """DeviceAdam.__init__ without its device check and struct of addresses: the param group alone (no GPU here)."""
    group = {"lr": float(lr), "betas": (float(betas[0]), float(betas[1])), "eps": float(eps), "max_grad_norm": float(max_grad_norm)}
    self._check_group(group)
    self.net, self.param_groups = net, [group]


def test_population_trainer_refuses_a_structural_difference_and_names_it(monkeypatch):
    from evacuation_amd import population, trainer
    monkeypatch.setattr(trainer.DeviceAdam, "__init__", _host_adam_init)
    pop = _cpu_population(3)
    base = RPOTrainingConfig(num_envs=2, num_steps=16, num_minibatches=4)
    import dataclasses
    cfgs = [base, dataclasses.replace(base, learning_rate=1e-3), dataclasses.replace(base, num_minibatches=8)]
    with pytest.raises(ValueError, match=r"num_minibatches.*learner 2"):
        population.PopulationTrainer(_FakeEnv(6), pop, cfgs)
    for field, value in (("num_steps", 32), ("update_epochs", 3), ("norm_adv", False), ("clip_vloss", False), ("total_timesteps", 64)):
        bad = [base, dataclasses.replace(base, **{field: value}), base]
        with pytest.raises(ValueError, match=field + r".*learner 1"):
            population.PopulationTrainer(_FakeEnv(6), pop, bad)
    with pytest.raises(ValueError, match="2 configurations for 3 learners"):
        population.PopulationTrainer(_FakeEnv(6), pop, cfgs[:2])
    ok = [base, dataclasses.replace(base, learning_rate=1e-3, gamma=0.9, anneal_lr=False, target_kl=0.01),
          dataclasses.replace(base, ent_coef=0.01, max_grad_norm=0.1)]
    tr = population.PopulationTrainer(_FakeEnv(6), pop, ok)
    assert tr.sweep and [g["lr"] for g in tr.optimizer.param_groups] == [3e-4, 1e-3, 3e-4]
    assert [g["max_grad_norm"] for g in tr.optimizer.param_groups] == [0.5, 0.5, 0.1]
    one = population.PopulationTrainer(_FakeEnv(6), pop, base)
    assert not one.sweep and one.cfg is base and one.optimizer.uniform()


# ------------------------------------------------------------------------------------------------ the compiled kernels
def _vgprs(kernels, stem):
    found = [k["vgpr_count"] for n, k in kernels.items() if stem in n]
    assert found, stem
    return max(found)


def _waves_per_simd(v):                                             # 512 VGPRs per SIMD lane, allocated in blocks of 8
    return min(8, 512 // ((v + 7) // 8 * 8))


def test_sweep_update_kernels_use_no_scratch_and_keep_the_register_class():
    mine = kernel_resources("evac_sweep_api.hip")
    one = kernel_resources("evac_train_api.hip")
    assert sorted(n.split("(")[0] for n in mine) == ["evac::k_sweep_advantages", "evac::k_sweep_finish", "evac::k_sweep_grad",
                                                    "evac::k_sweep_optimizer"], list(mine)
    assert not any(t in n for n in mine for t in ("k_gae", "k_adam", "k_rpo", "k_rollout", "k_step"))
    for name, k in mine.items():
        assert k["private_segment_fixed_size"] == 0 and k["vgpr_spill_count"] == 0, (name, k)
    for sibling, lone in (("k_sweep_grad", "k_rpo_grad"), ("k_sweep_optimizer", "k_adam"), ("k_sweep_finish", "k_rpo_finish"),
                          ("k_sweep_advantages", "k_gae")):
        assert _waves_per_simd(_vgprs(mine, sibling)) >= _waves_per_simd(_vgprs(one, lone)), (sibling, _vgprs(mine, sibling))


def test_sweep_collection_kernels_fit_the_register_budget():
    kernels = kernel_resources("evac_api.hip")
    mine = {n: k for n, k in kernels.items() if "k_collect_sweep" in n}
    assert len(mine) == 4, list(mine)                               # gravity / generic observation x default configuration or not
    for name, k in mine.items():
        assert k["vgpr_count"] <= 128 and k["vgpr_spill_count"] == 0 and k["private_segment_fixed_size"] == 0, (name, k)
        assert not any(t in name for t in ("k_collect_population", "k_rollout", "k_step", "k_policy_evaluate", "k_gae", "k_adam", "k_rpo"))
