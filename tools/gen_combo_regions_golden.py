#!/usr/bin/env python3
"""Writes tests/golden/kaori_combo_regions.json: what the reference's kaori::CombinatorialBarcodesSingleEnd<256, V> counts on
seeded cases with V = 1, 2, 3, 4, 5 and 8 variable regions.

Needs a checkout of the reference (--reference, its inst/include is read in place).  tools/combo_regions_driver.cpp is
compiled into a temporary directory outside the tree, run on every case in both modes, and only the JSON is kept.  Nothing
in the test suite or the build runs this tool.

    python tools/gen_combo_regions_golden.py --reference <screenCounter checkout>
"""
import argparse
import json
import os
import random
import shutil
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from tests import combo_regions_ref as ref  # noqa: E402
from tests import gen  # noqa: E402

OUT = os.path.join(ROOT, "tests", "golden", "kaori_combo_regions.json")
SEED = 23
MAX_BYTES = 400 * 1000


def specs(rng):
    """(name, keyword arguments of combo_regions_ref.make_case, what to break afterwards) per case."""
    out = []
    # every V with every strand and budget, short regions, pools of unequal sizes (one of them a single sequence)
    shapes = {1: [(8,), (12,)], 2: [(6, 9), (10, 4)], 3: [(5, 7, 6), (8, 3, 10)], 4: [(4, 6, 5, 7), (7, 3, 4, 5)], 5: [(4, 5, 3, 6, 4), (3, 4, 5, 3, 6)],
              8: [(3, 3, 3, 3, 3, 3, 3, 3), (4, 3, 5, 3, 4, 3, 3, 4)]}
    k = 0
    for V, lens_list in shapes.items():
        for lens in lens_list:
            for strand in (0, 1, 2):
                sizes = [[1, 2, 3, 5, 7, 4, 2, 6][(r + k) % 8] for r in range(V)]
                if V <= 3:
                    sizes = [s * 3 for s in sizes]
                    sizes[k % V] = 1
                out.append((f"V{V}", dict(lens=lens, sizes=sizes, n_reads=40, strand=strand, mismatches=k % 4,
                                           alphabet=("AC", "ACG", gen.BASES)[k % 3], iupac=(0, 0.06)[k % 2], begins=k % 5 == 1, ends=k % 5 == 3,
                                           p_sub=(0.0, 0.03, 0.08)[k % 3], p_n=(0, 0.02)[(k // 2) % 2], p_lower=(0, 0.3)[(k // 3) % 2]), None))
                k += 1
    # wide (33-64 bases) and big (65 and more) keys, alone and beside a short region
    for lens, mm in (((40, 6, 5), 2), ((8, 33), 1), ((64, 7, 34), 3), ((36,), 2), ((70, 5), 1), ((6, 100, 4), 2), ((65, 66, 8), 3), ((120,), 0), ((33, 33), 0), ((50,), 1),
                     ((10, 80, 12), 0), ((5, 5, 5, 5, 40), 2)):
        out.append(("wide" if max(lens) <= 64 else "big", dict(lens=lens, sizes=[3 + r for r in range(len(lens))], n_reads=24, strand=k % 3, mismatches=mm,
                                                                 iupac=(0, 0.03)[k % 2], flanks=(2, 8), begins=k % 4 == 0, ends=k % 4 == 2, p_sub=0.02, pad_hi=8), None))
        k += 1
    # two constructs per read and a low-complexity alphabet: first and best mode part ways
    for lens in ((4, 4, 4), (3, 5), (3, 3, 3, 3), (5,), (3, 4, 3)):
        out.append(("ties", dict(lens=lens, sizes=[4] * len(lens), n_reads=60, strand=2, mismatches=2, alphabet="AC", p_sub=0.1, flanks=(1, 3), pad_hi=20), None))
    # what the constructor rejects (:79-93)
    out.append(("rejected", dict(lens=(5, 6, 7), sizes=[3, 3, 3], n_reads=4, strand=0, mismatches=1), "drop a pool"))
    out.append(("rejected", dict(lens=(5, 6), sizes=[3, 3], n_reads=4, strand=2, mismatches=1), "add a pool"))
    out.append(("rejected", dict(lens=(5, 6, 7), sizes=[3, 3, 3], n_reads=4, strand=1, mismatches=0), "shorten pool 2"))
    out.append(("rejected", dict(lens=(5, 6, 7, 4), sizes=[2, 2, 2, 2], n_reads=4, strand=0, mismatches=2), "lengthen pool 4"))
    out.append(("rejected", dict(lens=(9,), sizes=[5], n_reads=4, strand=0, mismatches=0), "no region"))
    return out


def break_case(case, how, rng):
    if how == "drop a pool":
        case["pools"] = case["pools"][:-1]
    elif how == "add a pool":
        case["pools"] = case["pools"] + [gen.make_pool(rng, 2, 4, gen.BASES)]
    elif how == "shorten pool 2":
        case["pools"][1] = [s[:-1] for s in case["pools"][1]]
    elif how == "lengthen pool 4":
        case["pools"][3] = [s + "A" for s in case["pools"][3]]
    elif how == "no region":
        case["template"] = case["template"].replace("-", "A")


def write_fastq(path, reads):
    with open(path, "w") as f:
        for i, r in enumerate(reads):
            f.write(f"@r{i}\n{r}\n+\n{'I' * len(r)}\n")


def run(driver, tmp, case, use_first):
    fq, fp = os.path.join(tmp, "reads.fq"), os.path.join(tmp, "pools.txt")
    write_fastq(fq, case["reads"])
    with open(fp, "w") as f:
        for pool in case["pools"]:
            f.write(">\n" + "".join(p + "\n" for p in pool))
    out = subprocess.check_output([driver, fq, case["template"], str(case["strand"]), str(case["mismatches"]), str(int(use_first)), fp], text=True)
    head, _, body = out.partition("\n")
    word, _, rest = head.partition(" ")
    if word == "error":
        return {"error": rest.strip()}
    assert word == "ok", out
    total, k = (int(x) for x in rest.split())
    rows = [[int(x) for x in line.split()] for line in body.splitlines() if line.strip()]
    assert len(rows) == k, out
    return {"total": total, "combinations": rows}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reference", required=True, help="checkout of the reference (inst/include/kaori is read in place)")
    ap.add_argument("--cxx", default="g++")
    args = ap.parse_args()
    inc = os.path.join(args.reference, "inst", "include")
    if not os.path.isdir(os.path.join(inc, "kaori")):
        sys.exit(f"{inc}/kaori not found")
    tmp = tempfile.mkdtemp(prefix="combo_regions_golden_")
    try:
        driver = os.path.join(tmp, "combo_regions_driver")
        subprocess.check_call([args.cxx, "-O2", "-std=c++17", "-I" + inc, "-o", driver, os.path.join(ROOT, "tools", "combo_regions_driver.cpp"),
                               "-lz", "-lpthread"])
        rng = random.Random(SEED)
        cases, modes_differ, rejected = [], 0, 0
        for name, kwargs, how in specs(rng):
            for attempt in range(50):                 # (a case in which the handler counts nothing is drawn again)
                c = ref.make_case(rng, **kwargs)
                if how:
                    break_case(c, how, rng)
                c["source"] = f"{name}[{len(cases)}]"
                c["expect"] = {"first": run(driver, tmp, c, True), "best": run(driver, tmp, c, False)}
                if how or (c["expect"]["first"].get("combinations") and c["expect"]["best"].get("combinations")):
                    break                             # (so is one whose random IUPAC codes the handler rejects as duplicates)
            if "error" in c["expect"]["best"]:
                assert "error" in c["expect"]["first"] and how, c
                rejected += 1
            else:
                assert not how, (how, c["expect"])
                assert c["expect"]["first"]["combinations"] and c["expect"]["best"]["combinations"], c["source"]
                modes_differ += c["expect"]["first"]["combinations"] != c["expect"]["best"]["combinations"]
            cases.append(c)
        accepted = [c for c in cases if "error" not in c["expect"]["best"]]
        assert 4 * rejected <= len(cases), (rejected, len(cases))
        assert modes_differ >= 1, "first and best mode never differ"
        assert {len(c["pools"]) for c in accepted} == {1, 2, 3, 4, 5, 8}
        assert {c["strand"] for c in accepted} == {0, 1, 2} and {c["mismatches"] for c in accepted} == {0, 1, 2, 3}
        longest = [max(len(p[0]) for p in c["pools"]) for c in accepted]
        assert min(longest) <= 32 and any(32 < v <= 64 for v in longest) and max(longest) > 64
        assert any(c["template"].startswith("-") for c in accepted) and any(c["template"].endswith("-") for c in accepted)
        assert any(any(len(p) == 1 for p in c["pools"]) for c in accepted) and any(len({len(p) for p in c["pools"]}) > 1 for c in accepted)
        assert any(any(ch in gen.IUPAC for p in c["pools"] for s in p for ch in s) for c in accepted)
        text = json.dumps({"generator": "tools/gen_combo_regions_golden.py", "seed": SEED, "cases": cases}, separators=(",", ":"))
        assert len(text) <= MAX_BYTES, len(text)
        with open(OUT, "w") as f:
            f.write(text + "\n")
        print(f"{OUT}: {len(cases)} cases ({rejected} rejected by the reference), {sum(len(c['reads']) for c in cases)} reads, "
              f"first != best in {modes_differ}, {len(text)} bytes")
    finally:
        shutil.rmtree(tmp, ignore_errors=True)


if __name__ == "__main__":
    main()
