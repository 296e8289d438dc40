#!/usr/bin/env python3
"""Writes tests/golden/kaori_single_paired.json: what the reference's kaori::SingleBarcodePairedEnd counts on seeded cases.

Needs a checkout of the reference (--reference, its inst/include is read in place).  tools/single_paired_driver.cpp is
compiled into a temporary directory outside the tree, run on every case in both modes, and only the JSON is kept.  Nothing
in the test suite or the build runs this tool.

    python tools/gen_single_paired_golden.py --reference <screenCounter checkout>
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

from tests import single_paired_ref  # noqa: E402

OUT = os.path.join(ROOT, "tests", "golden", "kaori_single_paired.json")
SEED = 20
# (cases, keyword arguments of gen.random_single_case): barcodes of 1-32, 33-64 and 65-120 bases
GROUPS = [(22, dict(max_vlen=32)), (10, dict(min_vlen=33, max_vlen=64)), (8, dict(min_vlen=65, max_vlen=120))]
MAX_BYTES = 400 * 1000


def write_fastq(path, reads):
    with open(path, "w") as f:
        for i, r in enumerate(reads):
            f.write(f"@r{i}\n{r}\n+\n{'I' * len(r)}\n")


def run(driver, tmp, case, use_first):
    f1, f2, fp = (os.path.join(tmp, n) for n in ("m1.fq", "m2.fq", "pool.txt"))
    write_fastq(f1, case["reads1"])
    write_fastq(f2, case["reads2"])
    with open(fp, "w") as f:
        f.write("".join(p + "\n" for p in case["pool"]))
    out = subprocess.check_output([driver, f1, f2, case["template"], str(case["strand"]), str(case["mismatches"]), str(int(use_first)), fp],
                                  text=True).strip()
    word, _, rest = out.partition(" ")
    if word == "error":
        return {"error": rest}
    assert word == "ok", out
    numbers = [int(x) for x in rest.split()]
    return {"total": numbers[0], "counts": numbers[1:]}


def best_outcomes(driver, tmp, case, seen):
    """Which branches of the best-mode rule the case's pairs take, from the handler itself on one pair (or one mate) at a time."""
    for a, b in zip(case["reads1"], case["reads2"]):
        def hit(r1, r2, mm):
            got = run(driver, tmp, dict(case, reads1=[r1], reads2=[r2], mismatches=mm), False)["counts"]
            return got.index(1) if 1 in got else -1

        def best(read):            # the mate alone: the other mate is empty
            for mm in range(case["mismatches"] + 1):
                i = hit(read, "", mm)
                if i >= 0:
                    return i, mm
            return -1, None
        (i1, m1), (i2, m2) = best(a), best(b)
        if i1 < 0 or i2 < 0:
            continue
        pair = hit(a, b, case["mismatches"])
        if m1 < m2:
            assert pair == i1
            seen.add("mate 1 wins")
        elif m2 < m1:
            assert pair == i2
            seen.add("mate 2 wins")
        elif i1 == i2:
            assert pair == i1
            seen.add("equal, same index")
        else:
            assert pair == -1
            seen.add("equal, different indices")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reference", required=True, help="checkout of the reference (inst/include/kaori is read in place)")
    ap.add_argument("--cxx", default="g++")
    args = ap.parse_args()
    inc = os.path.join(args.reference, "inst", "include")
    if not os.path.isdir(os.path.join(inc, "kaori")):
        sys.exit(f"{inc}/kaori not found")
    tmp = tempfile.mkdtemp(prefix="single_paired_golden_")
    try:
        driver = os.path.join(tmp, "single_paired_driver")
        subprocess.check_call([args.cxx, "-O2", "-std=c++17", "-I" + inc, "-o", driver, os.path.join(ROOT, "tools", "single_paired_driver.cpp"),
                               "-lz", "-lpthread"])
        rng = random.Random(SEED)
        cases, seen, modes_differ, rejected = [], set(), 0, 0
        for n, kwargs in GROUPS:
            for _ in range(n):
                c = single_paired_ref.paired_case(rng, sizes=(1, 30, 60), **kwargs)
                c.pop("use_first")
                c["source"] = f"single_paired[{len(cases)}]"
                c["expect"] = {"first": run(driver, tmp, c, True), "best": run(driver, tmp, c, False)}
                if "error" in c["expect"]["best"]:
                    rejected += 1
                else:
                    modes_differ += c["expect"]["first"]["counts"] != c["expect"]["best"]["counts"]
                    if len(seen) < 4:
                        best_outcomes(driver, tmp, c, seen)
                cases.append(c)
        assert seen == {"mate 1 wins", "mate 2 wins", "equal, same index", "equal, different indices"}, seen
        assert modes_differ >= 1, "first and best mode never differ"
        assert {c["strand"] for c in cases} == {0, 1, 2} and {c["mismatches"] for c in cases} == {0, 1, 2, 3}
        text = json.dumps({"generator": "tools/gen_single_paired_golden.py", "seed": SEED, "cases": cases}, separators=(",", ":"))
        assert len(text) <= MAX_BYTES, len(text)
        with open(OUT, "w") as f:
            f.write(text + "\n")
        print(f"{OUT}: {len(cases)} cases ({rejected} rejected by the reference), {sum(len(c['reads1']) for c in cases)} pairs, "
              f"first != best in {modes_differ}, {len(text)} bytes")
    finally:
        shutil.rmtree(tmp, ignore_errors=True)


if __name__ == "__main__":
    main()
