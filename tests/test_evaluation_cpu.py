"""CPU checks of the policy evaluation (evac_policy_evaluate, evacuation_amd.evaluation, agents.WacuumCleaner): the ABI, the argument
checks that need no device, the scripted baseline against the reference's recorded actions, the kernels' resource budgets and
the summary arithmetic."""
import ctypes as C
import math
import os
import re

import numpy as np
import pytest

import evacuation_amd as ea
from evacuation_amd import _lib, build
from tests import evaluation_cases as EC
from tests.kernel_meta import kernel_resources

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def lib():
    build.build_library()
    return _lib.load()


def test_entry_is_declared_exported_and_bound(lib):
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "evac.h")).read(), flags=re.S)
    assert re.search(r"\bint\s+evac_policy_evaluate\s*\(", text)
    m = re.search(r"enum\s*\{\s*EVAC_AGENT_POLICY_MEAN\s*=\s*0\s*,\s*EVAC_AGENT_POLICY_SAMPLE\s*=\s*1\s*,\s*EVAC_AGENT_VACUUM_CLEANER\s*=\s*2\s*\}", text)
    assert m, "the agent codes of evac.h"
    assert (_lib.AGENT_POLICY_MEAN, _lib.AGENT_POLICY_SAMPLE, _lib.AGENT_VACUUM_CLEANER) == (0, 1, 2)
    res, args = _lib.SIGNATURES["evac_policy_evaluate"]
    assert res is C.c_int and len(args) == 11 and args[8] is C.c_float and args[9] is C.c_float
    assert lib.evac_policy_evaluate is not None
    assert lib.evac_version() == _lib.VERSION == 150
    for name in ("WacuumCleaner", "PolicyEvaluator", "EvaluationResult"):
        assert name in ea.__all__ and getattr(ea, name) is not None


def test_invalid_arguments_are_refused_without_a_device(lib):
    """Through the C entry with a NULL handle (every call is refused before anything could be launched), and through the Python
    checks that run before the library is reached."""
    words = (C.c_int32 * 4)()
    recs = (C.c_float * 10)()
    pol = _lib.EvacMlpPolicy(6, 64)                       # every tensor NULL
    for agent, policy, n_ep, steps, prog, out in (
            (0, C.byref(pol), 1, 1, words, recs),         # a NULL handle, whatever else is given
            (7, None, 1, 1, words, recs),                 # an unknown agent
            (2, None, 1, 1, None, recs), (2, None, 1, 1, words, None),      # NULL progress / episodes_out
            (2, None, 0, 1, words, recs), (2, None, 1, 0, words, recs),     # n_episodes / max_steps < 1
            (0, None, 1, 1, words, recs), (1, C.byref(pol), 1, 1, words, recs)):   # a policy agent without a policy / tensors
        assert lib.evac_policy_evaluate(None, agent, policy, n_ep, steps, prog, out, None, 1.0, 1e-8, None) == _lib.ERR_INVALID_ARGUMENT
    from evacuation_amd.vector_env import check_evaluate_args
    check_evaluate_args("vacuum_cleaner", 1, 1, None)     # fine
    check_evaluate_args(object(), 3, 17, ("norm_state", 1.0, 1e-8))
    for bad in (("rotating", 1, 1, None), (None, 1, 1, None), ("vacuum_cleaner", 0, 1, None), ("vacuum_cleaner", 1, 0, None),
                (object(), -1, 5, None), ("vacuum_cleaner", 1, 1, ("norm_state", 1.0, 1e-8))):
        with pytest.raises(ValueError):
            check_evaluate_args(*bad)
    # a network of the wrong width or observation dim never reaches the library: PolicyBinder refuses it
    import torch
    from evacuation_amd.policy import LinearActorCritic, PolicyBinder
    binder = PolicyBinder(6, torch.device("cpu"))
    with pytest.raises(ValueError, match="hidden width 32"):
        binder(LinearActorCritic(6, hidden=32))
    with pytest.raises(ValueError, match="observation dim"):
        binder(LinearActorCritic(7))


def test_wacuum_cleaner_reproduces_the_reference_actions():
    """Every recorded action of the reference's object from the recorded positions, bit for bit and dtype for dtype; a fresh
    agent at every episode start; the third phase is reached."""
    f = np.load(EC.GOLDEN)
    pos, act, start = f["positions"], f["actions"], f["episode_start"]
    assert pos.dtype == np.float32 and act.dtype == np.float32 and len(start) - 1 >= 3 and start[-1] == len(pos) >= 3000
    reached = []
    for ep in range(len(start) - 1):
        w, h, s = (float(v) for v in f["settings"][ep])
        agent = ea.WacuumCleaner(EC.fake_env(w, h, s))            # a fresh agent per episode
        for t in range(start[ep], start[ep + 1]):
            a = agent.act({"agent_position": pos[t]})
            assert a.dtype == np.float32 and a.shape == (2,), (ep, t)
            assert a.tobytes() == act[t].tobytes(), (ep, t, a, act[t])
        reached.append(agent.phase == agent.EXIT)
        assert reached[-1] == bool(f["third_task"][ep]), ep
        agent.reset()                                             # ... which reset() makes of a used one
        for t in range(start[ep], start[ep + 1]):
            assert agent.act({"agent_position": pos[t]}).tobytes() == act[t].tobytes(), (ep, t, "after reset()")
    assert any(reached)
    # no recorded position lies within an ulp of a threshold: float32 and float64 comparisons agree on this fixture
    for ep in range(len(start) - 1):
        w, h, s = (float(v) for v in f["settings"][ep])
        p = pos[start[ep]:start[ep + 1]].astype(np.float64)
        for thr, col in ((w - 0.1 + s, 0), (h - 0.1 + s, 1)):
            gap = np.abs(np.abs(p[:, col]) - thr).min()
            assert gap > np.spacing(np.float32(thr)), (ep, col, gap)


def test_device_thresholds_equal_the_host_agents():
    """The library holds the settings as float32 and reads them back as the shortest decimals that round to them (the Python
    floats a caller wrote); the host agent forms its turning points from the Python floats.  Restated here: the same float32
    for the settings of the fixture and of the GPU tests -- where the widened float32 values alone would differ."""
    def as_written(v32):
        for digits in range(1, 10):
            text = "%.*g" % (digits, float(v32))
            if np.float32(text) == v32:
                return float(text)
        return float(v32)
    f = np.load(EC.GOLDEN)
    settings = [tuple(float(v) for v in row) for row in f["settings"]] + [(1.0, 1.0, 0.01), (1.0, 1.0, 0.05)]
    widened_differs = 0
    for w, h, s in settings:
        agent = ea.WacuumCleaner(EC.fake_env(w, h, s))
        for ext, thr in ((w, agent.threshold_x), (h, agent.threshold_y)):
            assert as_written(np.float32(ext)) == ext and as_written(np.float32(s)) == s
            dev = np.float32(as_written(np.float32(ext)) - 0.2 / 2 + as_written(np.float32(s)))
            assert dev == thr and thr.dtype == np.float32, (w, h, s)
            widened_differs += np.float32(float(np.float32(ext)) - 0.2 / 2 + float(np.float32(s))) != thr
    assert widened_differs >= 1


def test_evaluate_kernels_fit_the_register_budget():
    kernels = {n: k for n, k in kernel_resources("evac_api.hip").items() if "k_policy_evaluate" in n}
    assert len(kernels) == EC.N_KERNELS, list(kernels)
    assert sum("k_policy_evaluate<" in n for n in kernels) == 8 and sum("k_policy_evaluate_scripted<" in n for n in kernels) == 2
    for name, k in kernels.items():
        assert k["vgpr_count"] <= 128 and k["vgpr_spill_count"] == 0 and k["private_segment_fixed_size"] == 0, (name, k)
    assert not any("k_policy_evaluate" in n for n in kernel_resources("evac_train_api.hip"))


def test_summary_of_a_hand_made_record_tensor():
    import torch
    from evacuation_amd.evaluation import EvaluationResult
    from evacuation_amd.vector_env import STATS_FIELDS, stats_int_view
    rec = torch.zeros((2, 3, 10), dtype=torch.float32)
    reward = torch.tensor([[1.0, 2.0, 3.0], [4.0, 5.0, 9.0]])
    length = torch.tensor([[10.0, 20.0, 30.0], [40.0, 50.0, 60.0]])
    escaped = torch.tensor([[4.0, 2.0, 0.0], [4.0, 4.0, 1.0]])
    rec[..., STATS_FIELDS.index("episode_reward")] = reward
    rec[..., STATS_FIELDS.index("episode_length")] = length
    rec[..., STATS_FIELDS.index("escaped_pedestrians")] = escaped
    stats_int_view(rec)[..., 0] = torch.tensor([[10, 20, 30], [50, 70, 90]], dtype=torch.int32)
    stats_int_view(rec)[..., 1] = torch.tensor([[1, 1, 1], [2, 2, 2]], dtype=torch.int32)
    res = EvaluationResult.from_records(rec, torch.tensor([50, 70, 90], dtype=torch.int32), n_pedestrians=4)
    assert set(STATS_FIELDS) | {"overall_timesteps", "n_episodes"} == set(res.episodes)
    assert res.episodes["n_episodes"].dtype == torch.int32 and res.episodes["n_episodes"].tolist() == [[1, 1, 1], [2, 2, 2]]
    assert tuple(res.episodes["episode_reward"].shape) == (2, 3)
    s = res.summary()
    assert all(type(v) in (float, int) for v in s.values())
    assert s["episodes"] == 6
    assert math.isclose(s["episode_reward_mean"], 4.0) and math.isclose(s["episode_reward_std"], math.sqrt(np.var([1, 2, 3, 4, 5, 9])))
    assert math.isclose(s["episode_length_mean"], 35.0)
    assert math.isclose(s["escaped_fraction_mean"], 15.0 / 24.0) and math.isclose(s["all_escaped_share"], 0.5)
