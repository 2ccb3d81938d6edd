"""CPU checks of the recording evaluation (evac_policy_evaluate*_capture, csrc/evac_capture_api.hip, policy_evaluate(capture=...),
EvaluationResult.episode_memory, trajectory.episode_to_memory): the existing units' kernel counts, the new unit's nine kernels and
their resources against their non-capturing counterparts, the ABI, the refusals that need no device, and one episode cut out of
hand-made frames."""
import ctypes as C
import os
import re
import subprocess
import tempfile
from enum import Enum
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import evacuation_amd as ea
from evacuation_amd import _lib, build
from evacuation_amd.statuses import Status

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = ("evac_policy_evaluate_capture", "evac_policy_evaluate_deepsets_capture", "evac_policy_evaluate_transformer_capture")
FIELDS = ("group_segment_fixed_size", "private_segment_fixed_size", "vgpr_count", "vgpr_spill_count")
LDS_LIMIT = 163840                                          # a CU's 160 KiB
# the nine kernels of evac_capture_api.hip and, of each, the non-capturing kernel it is held against (its unit, its name)
COUNTERPARTS = {
    **{f"void evac::k_evaluate_capture<{g}, {n}>": ("evac_api.hip", f"void evac::k_policy_evaluate<{g}, {n}, false>")
       for g in ("true", "false") for n in ("true", "false")},
    "evac::k_evaluate_capture_scripted": ("evac_api.hip", "void evac::k_policy_evaluate_scripted<false>"),
    **{f"void evac::k_evaluate_capture_{enc}<{n}>": (f"evac_{enc}_api.hip", f"void evac::k_policy_evaluate_{enc}<{n}, false>")
       for enc in ("deepsets", "transformer") for n in ("true", "false")},
}
# private_segment_fixed_size of the nine kernels, as measured: none of them has a stack
SCRATCH_BYTES = {name: 0 for name in COUNTERPARTS}


def kernel_metadata(source: str) -> dict:
    """tests/kernel_meta.kernel_resources with the static LDS beside the registers: {demangled kernel name without its
    arguments: {field: value}} of csrc/``source``, compiled with the product's own flags."""
    with tempfile.TemporaryDirectory() as tmp:
        out = os.path.join(tmp, "evac.s")
        flags = [f for f in build.FLAGS if f not in ("-fPIC", "-shared")]
        subprocess.run([build.hipcc_path()] + flags + ["-S", "--cuda-device-only", os.path.join(build.CSRC, source), "-o", out], check=True,
                       capture_output=True)
        text = open(out).read()
    meta = text[text.index("amdhsa.kernels:"):]
    kernels = {}
    for block in meta.split("  - .agpr_count:")[1:]:
        name = re.search(r"\.name:\s+(\S+)", block).group(1)
        kernels[name] = {k: int(re.search(rf"\.{k}:\s+(\d+)", block).group(1)) for k in FIELDS}
    names = subprocess.run(["c++filt"], input="\n".join(kernels), capture_output=True, text=True).stdout.splitlines()
    assert len(names) == len(kernels)
    return {n.split("(")[0]: v for n, v in zip(names, kernels.values())}


@pytest.fixture(scope="module")
def units():
    return {u: kernel_metadata(u) for u in ("evac_capture_api.hip", "evac_api.hip", "evac_deepsets_api.hip", "evac_transformer_api.hip")}


@pytest.fixture(scope="module")
def lib():
    build.build_library()
    return _lib.load()


def test_the_existing_units_keep_their_kernels(units):
    assert os.path.join(build.CSRC, "evac_capture_api.hip") == build.SOURCES[-1]
    assert sum("k_policy_evaluate" in n for n in units["evac_api.hip"]) == 10
    assert len(units["evac_transformer_api.hip"]) == 8 and len(units["evac_deepsets_api.hip"]) == 8
    for unit in ("evac_api.hip", "evac_deepsets_api.hip", "evac_transformer_api.hip"):
        assert not any("capture" in n for n in units[unit]), unit


def test_the_new_unit_has_nine_kernels_within_their_counterparts_budget(units):
    mine = units["evac_capture_api.hip"]
    assert sorted(mine) == sorted(COUNTERPARTS)
    for name, k in mine.items():
        unit, other = COUNTERPARTS[name]
        assert k["vgpr_count"] <= 128 and k["vgpr_spill_count"] == 0, (name, k)
        assert k["private_segment_fixed_size"] == SCRATCH_BYTES[name], (name, k)
        assert k["private_segment_fixed_size"] <= units[unit][other]["private_segment_fixed_size"] + 16, (name, k, units[unit][other])
        assert units[unit][other]["group_segment_fixed_size"] < k["group_segment_fixed_size"] <= LDS_LIMIT, (name, k)
    # the counterparts as the issue of this feature found them: no stack but the transformer's kernel with a normaliser
    for name, (unit, other) in COUNTERPARTS.items():
        want = 12 if other == "void evac::k_policy_evaluate_transformer<true, false>" else 0
        assert units[unit][other]["private_segment_fixed_size"] == want, other


def test_entries_are_declared_exported_and_bound(lib):
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "evac.h")).read(), flags=re.S)
    struct = re.search(r"typedef struct evac_eval_capture \{(.*?)\} evac_eval_capture_t;", text, flags=re.S)
    assert struct and re.findall(r"(\w+\*?)\s+(\w+);", struct.group(1)) == [
        ("int32_t", "capture_envs"), ("int32_t", "max_frames"), ("float*", "frames"), ("float*", "starts")]
    assert [f for f, _ in _lib.EvacEvalCapture._fields_] == ["capture_envs", "max_frames", "frames", "starts"]
    assert C.sizeof(_lib.EvacEvalCapture) == 24
    for name in ENTRIES:
        m = re.search(rf"\bint\s+{name}\s*\(([^;]*)\)\s*;", text)
        assert m, name
        res, args = _lib.SIGNATURES[name]
        assert res is C.c_int and len(args) == m.group(1).count(",") + 1, name
        assert getattr(lib, name) is not None
        # the counterpart's arguments word for word, with the capture in front of the stream
        counterpart = name[:-len("_capture")]
        theirs = re.search(rf"\bint\s+{counterpart}\s*\(([^;]*)\)\s*;", text).group(1)
        words = lambda s: re.sub(r"\s+", " ", s).strip()        # noqa: E731
        assert words(m.group(1)) == words(theirs.replace("void* stream", "const evac_eval_capture_t* capture, void* stream")), name
        assert args == _lib.SIGNATURES[counterpart][1][:-1] + [C.POINTER(_lib.EvacEvalCapture), C.c_void_p], name
    assert lib.evac_version() == _lib.VERSION == 150
    assert "episode_to_memory" in ea.__all__ and ea.episode_to_memory is not None
    assert [f.name for f in __import__("dataclasses").fields(ea.EvaluationResult)] == ["episodes", "steps", "n_pedestrians", "capture"]


def test_a_null_handle_is_an_invalid_argument(lib):
    words, recs, rows = (C.c_int32 * 4)(), (C.c_float * 10)(), (C.c_float * 33)()
    pol, sets, tf = _lib.EvacMlpPolicy(6, 64), _lib.EvacDeepSets(3, 24), _lib.EvacTransformer(3, 1, 3, 96, 0, 1e-5)
    cap = _lib.EvacEvalCapture(1, 1, C.cast(rows, C.c_void_p), C.cast(rows, C.c_void_p))
    front = (None, 0, C.byref(pol), 1, 1, words, recs, None, 1.0, 1e-8)
    assert lib.evac_policy_evaluate_capture(*front, C.byref(cap), None) == _lib.ERR_INVALID_ARGUMENT
    assert lib.evac_policy_evaluate_deepsets_capture(*front, C.byref(sets), C.byref(cap), None) == _lib.ERR_INVALID_ARGUMENT
    assert lib.evac_policy_evaluate_transformer_capture(*front, C.byref(tf), C.byref(cap), None) == _lib.ERR_INVALID_ARGUMENT


def test_the_python_faces_refuse_a_bad_capture_before_a_device_is_looked_for():
    from evacuation_amd.evaluation import PolicyEvaluator
    from evacuation_amd.vector_env import BatchedEvacuationEnv, check_evaluate_capture
    cpu, N, E = torch.device("cpu"), 10, 4
    env = SimpleNamespace(num_envs=E, n_ped=N, device=cpu)              # (no handle, no library: the checks come first)

    def cap(F=5, K=2, rows=N + 1, episodes=3, dtype=torch.float32, **over):
        return {"frames": torch.zeros((F, K, rows, 3), dtype=dtype), "starts": torch.zeros((episodes, K, rows, 3), dtype=dtype), **over}
    assert check_evaluate_capture(cap(), 3, E, N, cpu) == 2 and check_evaluate_capture(cap(K=E, F=1), 3, E, N, cpu) == E
    bad = {
        "K = 0": cap(K=0), "K > num_envs": cap(K=E + 1), "no frame": cap(F=0), "rows": cap(rows=N), "float64": cap(dtype=torch.float64),
        "starts of two episodes": cap(episodes=2), "starts of another K": cap(starts=torch.zeros((3, 3, N + 1, 3))),
        "three dimensions": cap(frames=torch.zeros((5, 2, 3 * (N + 1)))), "not contiguous": cap(frames=torch.zeros((5, 2, N + 1, 6))[..., ::2]),
        "a key missing": {"frames": torch.zeros((5, 2, N + 1, 3))}, "a tensor, not a dict": torch.zeros((5, 2, N + 1, 3)),
        "an array": cap(frames=np.zeros((5, 2, N + 1, 3), dtype=np.float32)),
    }
    for what, capture in bad.items():
        with pytest.raises(ValueError, match="capture"):
            check_evaluate_capture(capture, 3, E, N, cpu)
        for agent in ("vacuum_cleaner", object()):
            with pytest.raises(ValueError, match="capture"):
                BatchedEvacuationEnv.policy_evaluate(env, agent, 3, 7, capture=capture)
    # the population form records nothing, whatever the capture and before it looks at the population
    for capture in (cap(), bad["K = 0"]):
        with pytest.raises(ValueError, match="a capture cannot be given"):
            BatchedEvacuationEnv.policy_evaluate_population(env, object(), 3, 7, capture=capture)
    # PolicyEvaluator: K outside 0..num_envs and max_frames < 1, before a buffer is made
    ev = SimpleNamespace(env=SimpleNamespace(env_config=SimpleNamespace(max_timesteps=12), n_ped=N, device=cpu, obs_dim=36), num_envs=E)
    for kw in (dict(capture_envs=E + 1), dict(capture_envs=-1), dict(capture_envs=2, max_frames=0)):
        with pytest.raises(ValueError, match="capture_envs"):
            PolicyEvaluator.evaluate(ev, object(), 3, **kw)


class OtherStatus(Enum):
    A = 1
    B = 2
    C = 3
    D = 4


def _hand_made():
    """Two recorded envs of N = 3, three episodes of lengths 3, 1, 4 (env 0) and 2, 2, 1 (env 1): every float names its place."""
    N, K, F = 3, 2, 9
    lengths = torch.tensor([[3, 2], [1, 2], [4, 1]], dtype=torch.float32)
    f, k, i, c = torch.meshgrid(torch.arange(F), torch.arange(K), torch.arange(N + 1), torch.arange(3), indexing="ij")
    frames = (1000 * f + 100 * k + 10 * i + c).float() / 7                 # (sevenths: float32 values that float64 shows as they are)
    frames[:, :, :N, 2] = ((f + k + i)[:, :, :N, 0] % 4 + 1).float()       # statuses 1..4
    frames[:, :, N, 2] = 0.0
    starts = -frames[:3].clone() - 1.0
    starts[:, :, :N, 2] = ((f + 2 * k + 3 * i)[:3, :, :N, 0] % 4 + 1).float()
    frames[8, 1] = float("nan")                                            # env 1 took 5 steps: rows 5.. were never written
    rec = torch.zeros((3, 4, 10), dtype=torch.float32)                     # an evaluation batch of four envs, two recorded
    rec[:, :2, 1] = lengths
    rec[:, 2:, 1] = 5.0
    res = ea.EvaluationResult.from_records(rec, torch.tensor([8, 5, 15, 15], dtype=torch.int32), N)
    assert res.capture is None
    res.capture = {"frames": frames, "starts": starts}
    return res, frames, starts, lengths


def test_episode_memory_cuts_the_frames_at_the_episode_records():
    res, frames, starts, lengths = _hand_made()
    N = 3
    for env in range(2):
        first = 0
        for ep in range(3):
            L = int(lengths[ep, env])
            ped, agent = res.episode_memory(env, ep)
            assert sorted(ped) == ["positions", "statuses"] and list(agent) == ["position"]
            assert len(ped["positions"]) == len(ped["statuses"]) == L + 1 and len(agent["position"]) == L
            want = [starts[ep, env]] + [frames[first + t, env] for t in range(L)]          # the slice boundaries
            for got_pos, got_st, row in zip(ped["positions"], ped["statuses"], want):
                assert got_pos.dtype == np.float64 and got_pos.shape == (N, 2)
                assert got_pos.tobytes() == row[:N, :2].numpy().astype(np.float64).tobytes()
                assert got_st.shape == (N,) and all(type(s) is Status for s in got_st)
                assert [s.value for s in got_st] == [int(v) for v in row[:N, 2]]
            for got, row in zip(agent["position"], want[1:]):
                assert got.dtype == np.float32 and got.tobytes() == row[N, :2].numpy().tobytes()
            first += L
    # the reference's own enum, when it is the reference's drawing code that reads the lists
    ped, _ = res.episode_memory(1, 2, status_cls=OtherStatus)
    assert all(type(s) is OtherStatus for st in ped["statuses"] for s in st)
    assert [s.value for s in ped["statuses"][0]] == [int(v) for v in starts[2, 1, :N, 2]]
    # trajectory.episode_to_memory is the same cut, from the tensors themselves
    a = ea.episode_to_memory(frames, starts, lengths[:, 0], 0, 2)
    b = res.episode_memory(0, 2)
    assert all(x.tobytes() == y.tobytes() for x, y in zip(a[0]["positions"] + a[1]["position"], b[0]["positions"] + b[1]["position"]))


def test_episode_memory_refuses_what_was_not_recorded():
    res, frames, starts, lengths = _hand_made()
    for env, ep in ((2, 0), (3, 1), (-1, 0), (0, 3), (0, -1)):                 # envs 2 and 3 were not recorded; no episode 3
        with pytest.raises(IndexError):
            res.episode_memory(env, ep)
    res.episodes["episode_length"][2, 1] = 0.0                                 # env 1 has not finished its third episode
    with pytest.raises(IndexError):
        res.episode_memory(1, 2)
    assert len(res.episode_memory(1, 1)[1]["position"]) == 2
    short = ea.EvaluationResult(res.episodes, res.steps, 3, {"frames": frames[:7], "starts": starts})       # max_frames = 7
    assert len(short.episode_memory(0, 1)[1]["position"]) == 1                 # frames 3..3
    with pytest.raises(ValueError, match="max_frames"):
        short.episode_memory(0, 2)                                             # frames 4..7
    with pytest.raises(IndexError):
        ea.EvaluationResult(res.episodes, res.steps, 3).episode_memory(0, 0)   # nothing was recorded
