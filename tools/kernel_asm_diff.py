#!/usr/bin/env python3
"""Compare the gfx950 device assembly of two checkouts, kernel by kernel.

    python tools/kernel_asm_diff.py <checkout A> <checkout B> [--units evac_sweep_api.hip,...]

For every translation unit that both checkouts list in ``evacuation_amd.build.SOURCES`` (one that only one side has is named
and left out) the device code is compiled with
``build.FLAGS`` and ``-S --cuda-device-only``, as tests/kernel_meta.py does, and split per kernel: its code, its kernel
descriptor (.amdhsa_kernel .. .end_amdhsa_kernel) and its entry in the amdhsa.kernels metadata (the argument layout and the
resource figures).  Comments are dropped, the function number of block labels (.LBB<f>_<n> -> .LBB_<n>) and every mangled
symbol and section name are replaced by placeholders numbered in order of appearance within the kernel -- so a kernel that moved
in its file, or whose LDS variable now belongs to another function, still compares equal, and nothing else does.

Prints ``N of N identical`` per unit and in all, the names of kernels that only one side has, and a unified diff of every kernel
that differs; exits 1 on any difference.  A kernel that one side has as ``k(Args)`` and the other as the template instantiation
``k<>(Args)`` is named as renamed and compared like any other.  Pure text comparison: no instruction is looked for.
"""
import argparse
import concurrent.futures
import difflib
import importlib.util
import os
import re
import subprocess
import sys
import tempfile


def load_build(checkout):
    path = os.path.join(checkout, "evacuation_amd", "build.py")
    spec = importlib.util.spec_from_file_location("_build_" + str(abs(hash(path))), path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def device_asm(build, source):
    flags = [f for f in build.FLAGS if f not in ("-fPIC", "-shared")]
    with tempfile.TemporaryDirectory() as tmp:
        out = os.path.join(tmp, "unit.s")
        proc = subprocess.run([build.hipcc_path()] + flags + ["-S", "--cuda-device-only", source, "-o", out], capture_output=True,
                              text=True)
        if proc.returncode != 0:
            raise RuntimeError(f"hipcc failed on {source}:\n{proc.stderr}")
        with open(out) as f:
            return f.read()


SYMBOL = re.compile(r"\b(?:_Z\w+|__hip_cuid_\w+|\.L__unnamed_\d+|\.str(?:\.\d+)?)")


def normalise(lines):
    """Comments, block-label function numbers, symbol and section names out; one stripped line per line that says anything."""
    seen = {}
    out = []
    for line in lines:
        line = line.split(";", 1)[0].rstrip()
        if not line.strip():
            continue
        line = re.sub(r"\.LBB\d+_(\d+)", r".LBB_\1", line)
        line = re.sub(r"\.Lfunc_(begin|end)\d+", r".Lfunc_\1", line)
        line = re.sub(r"^(\s*\.section\s+)\S+", r"\1<section>", line)
        line = SYMBOL.sub(lambda m: seen.setdefault(m.group(0), f"<sym{len(seen)}>"), line)
        out.append(line.strip())
    return out


def split_kernels(text):
    """{mangled name: normalised lines of code + descriptor + metadata entry}"""
    lines = text.splitlines()
    names = [m.group(1) for m in (re.match(r"\s*\.amdhsa_kernel\s+(\S+)", l) for l in lines) if m]
    kernels = {}
    for name in names:
        start = next(i for i, l in enumerate(lines) if l.startswith(name + ":"))
        end = next(i for i in range(start, len(lines)) if lines[i].strip() == ".end_amdhsa_kernel")
        kernels[name] = lines[start:end + 1]
    # the metadata: the items of the amdhsa.kernels list, each from a line "  - .key:" at the list's own indentation to the next
    meta = text[text.index("amdhsa.kernels:"):].splitlines()[1:]
    items = []
    for line in meta:
        if re.match(r"  - \.", line):
            items.append([line])
        elif line.startswith("    ") and items:
            items[-1].append(line)
        elif line.strip():
            break                                      # the next top-level key (amdhsa.target, ...)
    for item in items:
        name = re.search(r"\.name:\s+(\S+)", "\n".join(item))
        if name:                                       # (a name without code compares as metadata alone)
            kernels[name.group(1)] = kernels.get(name.group(1), []) + ["<metadata>"] + item
    return {name: normalise(body) for name, body in kernels.items()}


def demangle(names):
    out = subprocess.run(["c++filt"], input="\n".join(names), capture_output=True, text=True).stdout.splitlines()
    return dict(zip(names, out)) if len(out) == len(names) else {n: n for n in names}


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("a", help="checkout A (the parent)")
    ap.add_argument("b", help="checkout B")
    ap.add_argument("--units", help="comma-separated file names under csrc/ (default: every unit of build.SOURCES)")
    ap.add_argument("--jobs", type=int, default=min(8, os.cpu_count() or 1))
    args = ap.parse_args()
    builds = [load_build(os.path.abspath(c)) for c in (args.a, args.b)]
    units = [[os.path.basename(s) for s in b.SOURCES] for b in builds]
    for side, other in ((0, 1), (1, 0)):                         # (a unit that one side adds or drops has nothing to be compared with)
        for u in units[side]:
            if u not in units[other]:
                print(f"only in {'AB'[side]}: {u}")
    chosen = args.units.split(",") if args.units else [u for u in units[1] if u in units[0]]
    with concurrent.futures.ThreadPoolExecutor(args.jobs) as pool:
        jobs = {(u, side): pool.submit(device_asm, builds[side], os.path.join(builds[side].CSRC, u)) for u in chosen for side in (0, 1)}
        asm = {key: split_kernels(job.result()) for key, job in jobs.items()}
    same_all = total_all = 0
    differs = False
    for u in chosen:
        ka, kb = asm[(u, 0)], asm[(u, 1)]
        names = demangle(sorted(set(ka) | set(kb)))
        # a kernel that became a template whose plain instantiation is the old kernel (k<>(Args) for k(Args)) is the same kernel
        # under another mangled name: B's is compared under A's name
        plain = lambda n: re.sub(r"^void ", "", names[n]).replace("<>", "")
        for nb in [n for n in kb if n not in ka]:
            for na in [n for n in ka if n not in kb]:
                if plain(na) == plain(nb) and names[na] != names[nb]:
                    print(f"  renamed: {names[na]} -> {names[nb]}")
                    kb[na] = kb.pop(nb)
                    break
        both = [n for n in ka if n in kb]
        same = [n for n in both if ka[n] == kb[n]]
        total = len(set(ka) | set(kb))
        print(f"{u}: {len(same)} of {total} identical")
        for n in ka:
            if n not in kb:
                print(f"  removed: {names[n]}")
        for n in kb:
            if n not in ka:
                print(f"  added: {names[n]}")
        for n in both:
            if ka[n] != kb[n]:
                print(f"  differs: {names[n]}")
                for line in difflib.unified_diff(ka[n], kb[n], "a", "b", lineterm="", n=2):
                    print("    " + line)
        same_all += len(same)
        total_all += total
        differs |= len(same) != total
    print(f"{same_all} of {total_all} identical")
    return 1 if differs else 0


if __name__ == "__main__":
    sys.exit(main())
