"""CPU checks of the evaluation of a population of deep-sets leaders (evac_policy_evaluate_population_deepsets):
the ABI, the unit's place in the build, and what the compiler made of its four kernels."""
import ctypes as C
import os
import re

import pytest

from evacuation_amd import _lib, build
from tests import kernel_meta

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
UNIT = "evac_deepsets_population_evaluate_api.hip"
ENTRY = "evac_policy_evaluate_population_deepsets"


@pytest.fixture(scope="module")
def lib():
    build.build_library()
    return _lib.load()


def test_entry_is_declared_exported_and_bound(lib):
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "evac.h")).read(), flags=re.S)
    m = re.search(r"\bint\s+" + ENTRY + r"\s*\(([^;]*)\)\s*;", text)
    assert m, "the declaration in evac.h"
    params = [p.strip() for p in m.group(1).split(",")]
    assert len(params) == 16
    assert "evac_mlp_policy_strides_t" in params[3] and "evac_deepsets_t" in params[4] and "evac_deepsets_strides_t" in params[5]
    assert "agent" in params[6] and "shared_episodes" in params[7] and "stream" in params[15]
    res, args = _lib.SIGNATURES[ENTRY]
    assert res is C.c_int and len(args) == 16 and args[13] is C.c_float and args[14] is C.c_float
    assert args[3] is C.POINTER(_lib.EvacMlpPolicyStrides) and args[4] is C.POINTER(_lib.EvacDeepSets)
    assert args[5] is C.POINTER(_lib.EvacDeepSetsStrides)
    assert getattr(lib, ENTRY) is not None
    assert lib.evac_version() == _lib.VERSION == 150
    # a NULL handle: refused before anything else is looked at, strides or no strides
    pol, st = _lib.EvacMlpPolicy(), _lib.EvacMlpPolicyStrides()
    enc, est = _lib.EvacDeepSets(), _lib.EvacDeepSetsStrides()
    call = getattr(lib, ENTRY)
    assert call(None, 2, None, None, None, None, 0, 1, 1, 1, None, None, None, 1.0, 1e-8, None) == _lib.ERR_INVALID_ARGUMENT
    assert call(None, 2, C.byref(pol), C.byref(st), C.byref(enc), C.byref(est), 0, 1, 1, 1, None, None, None, 1.0, 1e-8,
                None) == _lib.ERR_INVALID_ARGUMENT


def test_the_unit_is_built_before_the_recording_evaluation():
    names = [os.path.basename(s) for s in build.SOURCES]
    assert UNIT in names and names[-1] == "evac_capture_api.hip" and names.count(UNIT) == 1
    assert names.index(UNIT) > names.index("evac_deepsets_population_api.hip")
    assert os.path.join(build.CSRC, UNIT) in build.DEPENDS


def test_the_unit_holds_its_four_kernels_within_the_lone_kernels_budget(monkeypatch):
    monkeypatch.setattr(kernel_meta, "FIELDS", tuple(kernel_meta.FIELDS) + ("group_segment_fixed_size",))
    mine = kernel_meta.kernel_resources(UNIT)
    lone = {n: k for n, k in kernel_meta.kernel_resources("evac_deepsets_api.hip").items() if "k_policy_evaluate_deepsets<" in n}
    flags = [f"<{n}, {d}>" for n in ("true", "false") for d in ("true", "false")]
    stems = sorted(n.split("(")[0].replace("void ", "") for n in mine)
    assert stems == sorted("evac::k_evaluate_population_deepsets" + f for f in flags), stems
    assert len(lone) == 4
    for name, k in mine.items():
        assert k["private_segment_fixed_size"] == 0 and k["vgpr_spill_count"] == 0 and k["vgpr_count"] <= 128, (name, k)
        f = next(f for f in flags if f in name)
        twin = next(v for n, v in lone.items() if f in n)
        assert 0 < k["group_segment_fixed_size"] <= twin["group_segment_fixed_size"], (name, k, twin)   # (the pointer shifts need no LDS)
        assert k["group_segment_fixed_size"] <= 160 * 1024
    design = open(os.path.join(ROOT, "DESIGN.md")).read()
    assert "k_evaluate_population_deepsets" in design and ENTRY in design
