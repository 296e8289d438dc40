#!/usr/bin/env python3
"""Which LDS-staged kernel instantiations exist, and which of them a profiled run launched.  Runs on the CPU.

The staged kernels (scg_kernels.hip) are templates over the tile shape (NW, NT, NC), the key width and the kernel's
flags; the host picks one instantiation per batch.  This lists the instantiations of the product code object and,
given the kernel statistics of a run (``rocprofv3 --kernel-trace --stats``: the ``*_kernel_stats.csv`` file), says
which of them ran and which did not.

  tools/staged_variants.py                      # list the instantiations
  tools/staged_variants.py --stats run_kernel_stats.csv [-o report.txt]

The instantiations are read from the device code object bundled into screencounter_amd/libscg.so when it is there and
uncompressed; otherwise (or with --compile) scg_kernels.hip is compiled for the device alone (``--cuda-device-only -S``,
as tools/kernel_resources.sh does), which takes a few minutes.  Exit status 1 when a stats file is given and some
instantiation was not launched.
"""
from __future__ import annotations

import argparse
import csv
import os
import re
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FAMILIES = ("single_staged_kernel", "combo_staged_kernel", "dual_staged_kernel", "dual_passes_kernel", "random_staged_kernel")
_MANGLED = re.compile(rb"_ZN12_GLOBAL__N_1\d+(" + b"|".join(f.encode() for f in FAMILIES) + rb")I([A-Za-z0-9_]*?)EEv")
_ARG = re.compile(r"Li(\d+)E|Lb([01])E|([jm])")
_TYPES = {"j": "unsigned int", "m": "unsigned long"}


def _demangle_args(blob: str) -> str:
    out = []
    for m in _ARG.finditer(blob):
        if m.group(1) is not None:
            out.append(m.group(1))
        elif m.group(2) is not None:
            out.append("true" if m.group(2) == "1" else "false")
        else:
            out.append(_TYPES[m.group(3)])
    return ", ".join(out)


def variants_from_bytes(data: bytes) -> set[str]:
    """Instantiations named in a code object or an assembly listing, as 'family<args>' in demangled spelling."""
    return {f"{m.group(1).decode()}<{_demangle_args(m.group(2).decode())}>" for m in _MANGLED.finditer(data)}


def compile_variants() -> set[str]:
    src = os.path.join(ROOT, "screencounter_amd", "csrc", "scg_kernels.hip")
    with tempfile.TemporaryDirectory() as tmp:
        out = os.path.join(tmp, "k.s")
        subprocess.check_call(["/opt/rocm/bin/hipcc", "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-Wno-pass-failed",
                               "-I" + os.path.join(ROOT, "include"), "-I" + os.path.join(ROOT, "screencounter_amd", "csrc"),
                               "--cuda-device-only", "-S", "-o", out, src])
        with open(out, "rb") as f:
            return variants_from_bytes(f.read())


def product_variants(lib: str, force_compile: bool = False) -> tuple[set[str], str]:
    if not force_compile and os.path.exists(lib):
        with open(lib, "rb") as f:
            found = variants_from_bytes(f.read())
        if found:
            return found, os.path.relpath(lib, ROOT)
    return compile_variants(), "scg_kernels.hip (device-only compile)"


def launched(stats_csv: str) -> dict[str, int]:
    """'family<args>' -> calls, from a rocprofv3 kernel_stats.csv (demangled names)."""
    calls: dict[str, int] = {}
    pat = re.compile(r"(" + "|".join(FAMILIES) + r")<([^<>]*)>")
    with open(stats_csv, newline="") as f:
        for row in csv.DictReader(f):
            m = pat.search(row["Name"])
            if m:
                key = f"{m.group(1)}<{m.group(2)}>"
                calls[key] = calls.get(key, 0) + int(row["Calls"])
    return calls


def _order(v: str):
    fam, args = v.split("<", 1)
    return (FAMILIES.index(fam), [(0, int(a)) if a.isdigit() else (1, a) for a in args.rstrip(">").split(", ")])


def report(variants: set[str], source: str, calls: dict[str, int] | None, stats_name: str | None) -> tuple[str, int]:
    lines = [f"staged kernel instantiations in {source}: {len(variants)}"]
    for fam in FAMILIES:
        lines.append(f"  {fam}: {sum(v.startswith(fam + '<') for v in variants)}")
    missing = 0
    if calls is None:
        lines += [""] + sorted(variants, key=_order)
    else:
        ran = sorted((v for v in variants if calls.get(v)), key=_order)
        not_ran = sorted((v for v in variants if not calls.get(v)), key=_order)
        missing = len(not_ran)
        lines += ["", f"launched in {stats_name}: {len(ran)} of {len(variants)}", ""]
        lines += [f"launched      {calls[v]:6d}  {v}" for v in ran]
        lines += [f"NOT launched       0  {v}" for v in not_ran]
        extra = sorted(set(calls) - variants)
        if extra:
            lines += ["", "launched but not in the code object (stale stats?):"] + [f"  {v}" for v in extra]
    return "\n".join(lines) + "\n", missing


def main() -> int:
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--lib", default=os.path.join(ROOT, "screencounter_amd", "libscg.so"))
    ap.add_argument("--compile", action="store_true", help="compile scg_kernels.hip instead of reading libscg.so")
    ap.add_argument("--stats", help="rocprofv3 --kernel-trace --stats kernel_stats.csv")
    ap.add_argument("-o", "--output", help="write the report here as well")
    a = ap.parse_args()
    variants, source = product_variants(a.lib, a.compile)
    calls = launched(a.stats) if a.stats else None
    text, missing = report(variants, source, calls, os.path.basename(a.stats) if a.stats else None)
    sys.stdout.write(text)
    if a.output:
        with open(a.output, "w") as f:
            f.write(text)
    return 1 if missing else 0


if __name__ == "__main__":
    sys.exit(main())
