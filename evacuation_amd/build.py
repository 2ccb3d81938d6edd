"""Build libevac.so (HIP, gfx950) in-tree with hipcc.  `python -m evacuation_amd.build [--force]`."""
from __future__ import annotations

import os
import shutil
import subprocess
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(HERE, "csrc")
LIB_PATH = os.path.join(HERE, "libevac.so")
# the env | the trainer's update | the update of a population of learners | ... with a configuration per learner | the deep-sets leader
# | its gradient | its optimiser step and whole update | the transformer leader | its gradient | its optimiser step and whole
# update | a population of deep-sets leaders | its evaluation | a population of transformer leaders: its collection | its
# evaluation | its update | a sweep of deep-sets leaders | of transformer leaders | the recording evaluation
SOURCES = [os.path.join(CSRC, f) for f in ("evac_api.hip", "evac_train_api.hip", "evac_population_api.hip", "evac_sweep_api.hip",
                                           "evac_deepsets_api.hip", "evac_deepsets_train_api.hip",
                                           "evac_deepsets_update_api.hip", "evac_transformer_api.hip",
                                           "evac_transformer_train_api.hip", "evac_transformer_update_api.hip",
                                           "evac_deepsets_population_api.hip", "evac_deepsets_population_evaluate_api.hip",
                                           "evac_transformer_population_api.hip", "evac_transformer_population_evaluate_api.hip",
                                           "evac_transformer_population_update_api.hip", "evac_deepsets_sweep_api.hip",
                                           "evac_transformer_sweep_api.hip", "evac_capture_api.hip")]
# what the library is built from: every source and header under csrc/, and the public header last
DEPENDS = sorted(os.path.join(CSRC, f) for f in os.listdir(CSRC) if f.endswith((".h", ".hip"))) + [
    os.path.join(os.path.dirname(HERE), "include", "evac.h")]
ARCH = "gfx950"
# -ffp-contract=off: fused multiply-adds are written explicitly in the kernels, so the f32 arithmetic
# is the same IEEE operation sequence as the NumPy f32 oracle wherever both use the same formula.
# -fno-slp-vectorize: the packed-f32 arithmetic of the kernels is written explicitly (v_pk_* through vector types and inline
# asm); what the SLP vectoriser adds on top are pairs built with v_mov shuffles around scalar code (-1 % at C2, A/B in
# profiles/r04_a_c2_ab_tile_layout_salu_diet_driver_args.txt: lib_v1 / lib_v1n).
FLAGS = ["-O3", f"--offload-arch={ARCH}", "-ffp-contract=off", "-fno-slp-vectorize", "-std=c++17", "-fPIC", "-shared"]


def hipcc_path() -> str:
    for cand in (os.environ.get("HIPCC"), shutil.which("hipcc"), "/opt/rocm/bin/hipcc"):
        if cand and os.path.exists(cand):
            return cand
    raise RuntimeError("hipcc not found (set HIPCC or install ROCm)")


def is_stale() -> bool:
    if not os.path.exists(LIB_PATH):
        return True
    t = os.path.getmtime(LIB_PATH)
    return any(os.path.getmtime(d) > t for d in DEPENDS)


def build_library(force: bool = False, verbose: bool = False) -> str:
    if not force and not is_stale():
        return LIB_PATH
    cmd = [hipcc_path()] + FLAGS + SOURCES + ["-o", LIB_PATH]
    if verbose:
        print(" ".join(cmd), flush=True)
    proc = subprocess.run(cmd, capture_output=True, text=True)
    if proc.returncode != 0:
        raise RuntimeError("hipcc failed:\n" + proc.stdout + proc.stderr)
    return LIB_PATH


if __name__ == "__main__":
    print(build_library(force="--force" in sys.argv, verbose=True))
