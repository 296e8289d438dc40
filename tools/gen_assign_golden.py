#!/usr/bin/env python3
"""Writes tests/golden/kaori_assign.json: the State the reference's kaori::SimpleSingleMatch leaves for every read of seeded
cases, in first and in best mode.

Needs a checkout of the reference (--reference, its inst/include is read in place).  tools/assign_driver.cpp is compiled
into a temporary directory outside the tree, run on every case in both modes, and only the JSON is kept.  Nothing in the
test suite or the build runs this tool.

    python tools/gen_assign_golden.py --reference <screenCounter checkout>
    python tools/gen_assign_golden.py --reference <screenCounter checkout> --check-edges

--check-edges writes no golden: it runs every read of every batch of tests/assign_cases.py (inputs whose expected states
follow from how they were built) through the same driver, asserts that the reference gives exactly those states, and
writes the tally to profiles/assign_edges_vs_kaori.txt.
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

from tests import gen  # noqa: E402

OUT = os.path.join(ROOT, "tests", "golden", "kaori_assign.json")
EDGES_OUT = os.path.join(ROOT, "profiles", "assign_edges_vs_kaori.txt")
SEED = 31
FIELDS = ("index", "position", "mismatches", "variable_mismatches", "reverse")
# (group, cases, keyword arguments of gen.random_single_case): barcodes of 1-32, 33-64 and 65-120 bases as ragged batches;
# then cases whose reads are padded or cut to one length (counted with fixed_len), and cases whose reads are padded to
# 321 bases and more (beyond the staged tiles)
GROUPS = [("short", 22, dict(max_vlen=32, sizes=(1, 30, 60))), ("wide", 10, dict(min_vlen=33, max_vlen=64, sizes=(1, 30, 60))),
          ("big", 8, dict(min_vlen=65, max_vlen=120, sizes=(1, 30, 60))),
          ("fixed", 4, dict(max_vlen=32, sizes=(30,))), ("long", 2, dict(max_vlen=32, sizes=(30,)))]
MIN_ACCEPTED = 35           # of the 40 cases of the first three groups
MAX_BYTES = 400 * 1000


def run(driver, tmp, template, strand, mismatches, pool, reads, use_first):
    """The driver's answer: {"error": message} or one list per field."""
    fr, fp = os.path.join(tmp, "reads.txt"), os.path.join(tmp, "pool.txt")
    with open(fr, "w") as f:
        f.write("".join(r + "\n" for r in reads))
    with open(fp, "w") as f:
        f.write("".join(p + "\n" for p in pool))
    out = subprocess.check_output([driver, fr, template, str(strand), str(mismatches), str(int(use_first)), fp], text=True)
    if out.startswith("error "):
        return {"error": out[len("error "):].strip()}
    rows = [[int(x) for x in line.split()] for line in out.splitlines()]
    assert len(rows) == len(reads) and all(len(r) == 5 for r in rows), (len(rows), len(reads))
    return {f: [r[k] for r in rows] for k, f in enumerate(FIELDS)}


def reshape(rng, case, group):
    """The reads of a `fixed` case at one length (cut, or padded with random bases on either side), those of a `long` case
    padded to 321..400 bases."""
    T = len(case["template"])
    if group == "fixed":
        L = case["fixed_len"] = T + rng.choice([0, 3, 17])
        out = []
        for r in case["reads"]:
            if len(r) > L:
                a = rng.randint(0, len(r) - L)
                r = r[a:a + L]
            else:
                a = rng.randint(0, L - len(r))
                r = gen.rand_seq(rng, a) + r + gen.rand_seq(rng, L - len(r) - a)
            out.append(r)
        case["reads"] = out
    elif group == "long":
        out = []
        for i, r in enumerate(case["reads"]):
            L = max(len(r), rng.randint(321, 400)) if i % 4 else len(r)       # (every fourth read stays as it is)
            a = rng.randint(0, L - len(r))
            out.append(gen.rand_seq(rng, a) + r + gen.rand_seq(rng, L - len(r) - a))
        case["reads"] = out
        assert max(len(r) for r in out) >= 321


def coverage(cases):
    """The conditions the golden must meet (tests/test_assign_abi.py asserts them again from the file)."""
    ok = [c for c in cases if "error" not in c["expect"]["first"]]
    main = [c for c in cases if c["group"] in ("short", "wide", "big")]
    assert len(main) == 40 and sum("error" not in c["expect"]["first"] for c in main) >= MIN_ACCEPTED
    assert {c["strand"] for c in cases} == {0, 1, 2} and {c["mismatches"] for c in cases} == {0, 1, 2, 3}
    seen = set()
    for c in ok:
        first, best = c["expect"]["first"], c["expect"]["best"]
        if first != best:
            seen.add("first != best")
        for e in (first, best):
            for i, p, m, v, r in zip(*(e[f] for f in FIELDS)):
                if i < 0:
                    assert (i, p, m, v, r) == (-1, -1, -1, -1, -1)
                    continue
                assert 0 <= v <= m <= c["mismatches"] and r in (0, 1) and p >= 0
                seen.add("reverse" if r else "forward")
                if p > 0:
                    seen.add("position > 0")
                if v < m:
                    seen.add("variable < total")
                if v == m and m > 0:
                    seen.add("variable == total > 0")
        if any(a >= 0 and b < 0 for a, b in zip(first["index"], best["index"])):
            seen.add("tie")
    want = {"first != best", "forward", "reverse", "position > 0", "variable < total", "variable == total > 0", "tie"}
    assert seen == want, want - seen
    return len(ok)


def write_golden(driver, tmp, seed):
    rng = random.Random(seed)
    cases = []
    for group, n, kwargs in GROUPS:
        for _ in range(n):
            c = gen.random_single_case(rng, **kwargs)
            c.pop("use_first")
            c.pop("kind")
            c["group"] = group
            c["source"] = f"assign[{len(cases)}]"
            reshape(rng, c, group)
            args = (c["template"], c["strand"], c["mismatches"], c["pool"], c["reads"])
            c["expect"] = {"first": run(driver, tmp, *args, True), "best": run(driver, tmp, *args, False)}
            cases.append(c)
    accepted = coverage(cases)
    differ = sum(c["expect"]["first"] != c["expect"]["best"] for c in cases)
    text = json.dumps({"generator": "tools/gen_assign_golden.py", "seed": seed, "fields": FIELDS, "cases": cases}, separators=(",", ":"))
    assert len(text) <= MAX_BYTES, len(text)
    with open(OUT, "w") as f:
        f.write(text + "\n")
    print(f"{OUT}: {len(cases)} cases ({len(cases) - accepted} rejected by the reference), {sum(len(c['reads']) for c in cases)} reads, "
          f"first != best in {differ}, {len(text)} bytes")


def check_edges(driver, tmp):
    from tests import assign_cases as A
    lines = ["# The constructed inputs of tests/assign_cases.py against kaori::SimpleSingleMatch (tools/assign_driver.cpp): every read of",
             "# every batch in first and in best mode, the expected state (by construction) against the reference's, field by field.",
             "#   python tools/gen_assign_golden.py --reference <checkout> --check-edges",
             "# cell | budget | reads of interest | batches | reads run per mode | differences first | differences best"]
    total_reads = total_diff = 0
    for cell in A.CELLS:
        case = A.case(cell)
        diffs = []
        n_reads = 0
        for use_first in (True, False):
            bad = 0
            for batch in case.batches:
                got = run(driver, tmp, case.template, A.STRAND, case.budget, case.pool, case.reads(batch), use_first)
                assert "error" not in got, (cell["id"], got)
                exp = case.expected(batch, use_first)
                n_reads += len(batch)
                for k, f in enumerate(FIELDS):
                    for r, (a, b) in enumerate(zip(exp[k].tolist(), got[f])):
                        if a != b:
                            bad += 1
                            print(f"{cell['id']} use_first={use_first} {case.items[batch[r]][0]}: {f} expected {a}, kaori {b}", file=sys.stderr)
            diffs.append(bad)
        lines.append(f"{cell['id']} | {case.budget} | {len(case.items)} | {len(case.batches)} | {n_reads // 2} | {diffs[0]} | {diffs[1]}")
        total_reads += n_reads
        total_diff += sum(diffs)
    lines.append(f"# {len(A.CELLS)} cells, {total_reads} reads run over both modes, {total_diff} differences")
    with open(EDGES_OUT, "w") as f:
        f.write("\n".join(lines) + "\n")
    print(lines[-1])
    assert total_diff == 0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reference", required=True, help="checkout of the reference (inst/include/kaori is read in place)")
    ap.add_argument("--cxx", default="g++")
    ap.add_argument("--seed", type=int, default=SEED, help="the committed golden uses the default")
    ap.add_argument("--check-edges", action="store_true", help="verify tests/assign_cases.py against the reference instead of writing the golden")
    args = ap.parse_args()
    inc = os.path.join(args.reference, "inst", "include")
    if not os.path.isdir(os.path.join(inc, "kaori")):
        sys.exit(f"{inc}/kaori not found")
    tmp = tempfile.mkdtemp(prefix="assign_golden_")
    try:
        driver = os.path.join(tmp, "assign_driver")
        subprocess.check_call([args.cxx, "-O2", "-std=c++17", "-I" + inc, "-o", driver, os.path.join(ROOT, "tools", "assign_driver.cpp")])
        if args.check_edges:
            check_edges(driver, tmp)
        else:
            write_golden(driver, tmp, args.seed)
    finally:
        shutil.rmtree(tmp, ignore_errors=True)


if __name__ == "__main__":
    main()
