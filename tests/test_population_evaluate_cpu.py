"""CPU checks of the population evaluation (evac_policy_evaluate_population, evaluation.PopulationEvaluator,
EvaluationResult.summaries): the kernels' resource budgets, the ABI, the one-transfer summaries and the argument checks that need
no device."""
import ctypes as C
import os
import re

import pytest

import evacuation_amd as ea
from evacuation_amd import _lib, build
from tests.kernel_meta import kernel_resources

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def lib():
    build.build_library()
    return _lib.load()


def test_population_evaluation_kernels_fit_the_register_budget():
    kernels = kernel_resources("evac_api.hip")
    mine = {n: k for n, k in kernels.items() if "k_evaluate_population<" in n}
    assert len(mine) == 8, list(mine)                               # gravity / generic observation x frozen norm or not x default config or not
    for name, k in mine.items():
        assert k["vgpr_count"] <= 128 and k["vgpr_spill_count"] == 0 and k["private_segment_fixed_size"] == 0, (name, k)
        assert not any(t in name for t in ("k_collect", "k_rollout", "k_step", "k_policy_evaluate"))   # (the other tests' counts stand)


def test_entry_is_declared_exported_and_bound(lib):
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "evac.h")).read(), flags=re.S)
    m = re.search(r"\bint\s+evac_policy_evaluate_population\s*\(([^;]*)\)\s*;", text)
    assert m, "the declaration in evac.h"
    params = [p.strip() for p in m.group(1).split(",")]
    assert len(params) == 14 and "shared_episodes" in params[5] and "evac_mlp_policy_strides_t" in params[3]
    res, args = _lib.SIGNATURES["evac_policy_evaluate_population"]
    assert res is C.c_int and len(args) == 14 and args[11] is C.c_float and args[12] is C.c_float
    assert args[3] is C.POINTER(_lib.EvacMlpPolicyStrides)
    assert lib.evac_policy_evaluate_population is not None
    assert lib.evac_version() == _lib.VERSION == 150
    assert "PopulationEvaluator" in ea.__all__ and ea.PopulationEvaluator is not None
    # a NULL handle: refused before anything else is looked at
    assert lib.evac_policy_evaluate_population(None, 2, None, None, 0, 1, 1, 1, None, None, None, 1.0, 1e-8, None) == _lib.ERR_INVALID_ARGUMENT


def hand_made_records():
    """[K, S, E, 10] = [2, 3, 4, 10] with different rewards, lengths and escapes per learner; n_pedestrians = 4."""
    import torch
    from evacuation_amd.vector_env import STATS_FIELDS, stats_int_view
    K, S, E = 2, 3, 4
    g = torch.Generator().manual_seed(3)
    rec = torch.zeros((K, S, E, 10), dtype=torch.float32)
    rec[..., STATS_FIELDS.index("episode_reward")] = torch.randn((K, S, E), generator=g) * 3.0 + torch.arange(S).reshape(1, S, 1)
    rec[..., STATS_FIELDS.index("episode_length")] = torch.randint(1, 30, (K, S, E), generator=g).float()
    rec[..., STATS_FIELDS.index("escaped_pedestrians")] = torch.randint(0, 5, (K, S, E), generator=g).float()
    stats_int_view(rec)[..., 1] = torch.arange(1, K + 1, dtype=torch.int32).reshape(K, 1, 1)
    return rec


def test_summaries_equal_the_summary_of_every_learner():
    import torch
    from evacuation_amd.evaluation import EvaluationResult
    from evacuation_amd.vector_env import STATS_FIELDS
    rec = hand_made_records()
    K, S, E = rec.shape[:3]
    steps = torch.arange(S * E, dtype=torch.int32).reshape(S, E)
    results = [EvaluationResult.from_records(rec[:, s], steps[s], n_pedestrians=4) for s in range(S)]
    both = EvaluationResult.summaries(results)
    assert both == [res.summary() for res in results]
    assert len(both) == S and all(type(v) in (float, int) for d in both for v in d.values())
    assert all(d["episodes"] == K * E for d in both)
    assert len({d["episode_reward_mean"] for d in both}) == S       # (the learners are told apart)
    # ... and the views' values are those of a learner's own contiguous records
    for s in range(S):
        alone = EvaluationResult.from_records(rec[:, s].contiguous(), steps[s], n_pedestrians=4).summary()
        assert alone == both[s], s
    esc = rec[:, 1, :, STATS_FIELDS.index("escaped_pedestrians")]
    assert both[1]["all_escaped_share"] == float((esc == 4).double().mean())
    assert EvaluationResult.summaries([]) == []


def test_population_evaluator_refuses_before_a_handle_exists():
    import torch
    from evacuation_amd.evaluation import PopulationEvaluator, check_population_norm_state
    cfg = ea.EnvConfig(number_of_pedestrians=10)
    for S, E in ((0, 4), (65, 4), (2, 0), (-1, 4)):
        with pytest.raises(ValueError):
            PopulationEvaluator(cfg, None, num_learners=S, num_envs=E, device="cuda:0")
    D, W = 6, 22
    good = torch.zeros((3, 5, W), dtype=torch.float64)
    parts = check_population_norm_state(good, 3, D)
    assert len(parts) == 3 and all(tuple(t.shape) == (5, W) for t in parts)
    ragged = [torch.zeros((1, W), dtype=torch.float64), torch.zeros((5, W), dtype=torch.float64), torch.zeros((2, W), dtype=torch.float64)]
    assert len(check_population_norm_state(ragged, 3, D)) == 3       # a learner's own number of rows
    for bad in (torch.zeros((2, 5, W), dtype=torch.float64),        # another number of learners
                torch.zeros((5, W), dtype=torch.float64),           # one learner's statistics where S are expected
                torch.zeros((3, 5, W + 1), dtype=torch.float64),    # another observation width
                torch.zeros((3, 5, W), dtype=torch.float32),        # not float64
                torch.zeros((3, 0, W), dtype=torch.float64),        # no rows
                ragged[:2], ragged[:2] + [None], "norm", 7):
        with pytest.raises(ValueError):
            check_population_norm_state(bad, 3, D)
