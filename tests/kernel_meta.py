"""The resource figures of the compiled kernels of one source file, read from the metadata of its gfx950 assembly."""
import os
import re
import subprocess
import tempfile

from evacuation_amd import build

CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "evacuation_amd", "csrc")
FIELDS = ("vgpr_count", "vgpr_spill_count", "sgpr_count", "sgpr_spill_count", "private_segment_fixed_size")


def kernel_resources(source: str) -> dict:
    """Compile the device code of csrc/``source`` with the product's own flags; {demangled kernel name: {field: value}} for
    ``FIELDS``, in the order of the assembly's metadata."""
    with tempfile.TemporaryDirectory() as tmp:
        out = os.path.join(tmp, "evac.s")
        flags = [f for f in build.FLAGS if f not in ("-fPIC", "-shared")]
        subprocess.run([build.hipcc_path()] + flags + ["-S", "--cuda-device-only", os.path.join(CSRC, source), "-o", out], check=True,
                       capture_output=True)
        text = open(out).read()
    meta = text[text.index("amdhsa.kernels:"):]
    kernels = {}
    for block in meta.split("  - .agpr_count:")[1:]:
        name = re.search(r"\.name:\s+(\S+)", block).group(1)
        kernels[name] = {k: int(re.search(rf"\.{k}:\s+(\d+)", block).group(1)) for k in FIELDS}
    names = subprocess.run(["c++filt"], input="\n".join(kernels), capture_output=True, text=True).stdout.splitlines()
    assert len(names) == len(kernels)
    return dict(zip(names, kernels.values()))
