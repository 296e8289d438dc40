"""scg_assign_batch (kaori::SimpleSingleMatch::State per read) without a GPU: the symbol is declared, exported and bound;
its argument errors come before any device work; the golden file of tools/gen_assign_golden.py
(tests/golden/kaori_assign.json, kaori's own results) covers what it was generated to cover; and both that golden and the
constructed edge cases of tests/assign_cases.py agree with the oracle every other test trusts: the barcodes they assign
add up to oracle.count_single's counts on the same reads."""
import json
import os
import re

import numpy as np
import pytest

from tests import assign_cases as A
from tests import golden_util as G

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIELDS = ("index", "position", "mismatches", "variable_mismatches", "reverse")
CASES = G.load("kaori_assign.json")
ACCEPTED = [c for c in CASES if "error" not in c["expect"]["first"]]


def test_symbol_is_declared_exported_and_bound(sc):
    from screencounter_amd import _lib
    header = open(os.path.join(ROOT, "include", "scg.h")).read()
    assert re.search(r"\bint scg_assign_batch\(", header)
    assert "SimpleSingleMatch.hpp:103-140" in header and ":200-306" in header
    assert hasattr(sc.load(), "scg_assign_batch") and "scg_assign_batch" in _lib.SIGNATURES
    assert hasattr(sc.Plan, "assign") and hasattr(sc, "assign_single_barcodes")
    assert sc.Assignment._fields == FIELDS


def test_null_plan(sc):
    from screencounter_amd import _lib
    L, err = sc.load(), _lib.errbuf()
    assert L.scg_assign_batch(None, None, None, 12, 12, 1, None, None, None, None, None, None, err, _lib.ERRCAP) == _lib.SCG_ERR_INVALID
    assert err.value == b"null plan"
    assert L.scg_assign_batch(None, None, None, 12, 12, 0, None, None, None, None, None, None, err, _lib.ERRCAP) == _lib.SCG_ERR_INVALID
    assert err.value == b"null plan"


def test_golden_file_covers_what_it_was_generated_for():
    with open(os.path.join(G.GOLDEN, "kaori_assign.json")) as f:
        text = f.read()
    doc = json.loads(text)
    assert len(text) <= 400 * 1000 and doc["generator"] == "tools/gen_assign_golden.py" and isinstance(doc["seed"], int)
    assert tuple(doc["fields"]) == FIELDS
    groups = [c["group"] for c in CASES]
    assert [groups.count(g) for g in ("short", "wide", "big", "fixed", "long")] == [22, 10, 8, 4, 2]
    for c in CASES:
        klen = c["template"].count("-")
        lo, hi = {"short": (1, 32), "wide": (33, 64), "big": (65, 120), "fixed": (1, 32), "long": (1, 32)}[c["group"]]
        assert lo <= klen <= hi, c["source"]
        if c["group"] == "fixed":
            assert {len(r) for r in c["reads"]} == {c["fixed_len"]}
        if c["group"] == "long":
            assert max(len(r) for r in c["reads"]) >= 321
    main = [c for c in CASES if c["group"] in ("short", "wide", "big")]
    assert sum("error" not in c["expect"]["first"] for c in main) >= 35
    assert {c["strand"] for c in CASES} == {0, 1, 2} and {c["mismatches"] for c in CASES} == {0, 1, 2, 3}
    seen = set()
    for c in CASES:
        first, best = c["expect"]["first"], c["expect"]["best"]
        assert ("error" in first) == ("error" in best)
        if "error" in first:
            assert first == best
            continue
        if first != best:
            seen.add("first != best")
        for e in (first, best):
            assert all(len(e[f]) == len(c["reads"]) for f in FIELDS)
            for i, p, m, v, r in zip(*(e[f] for f in FIELDS)):
                if i < 0:
                    assert (i, p, m, v, r) == A.NONE
                    continue
                assert i < len(c["pool"]) and 0 <= v <= m <= c["mismatches"] and r in (0, 1) and p >= 0
                seen.add("reverse" if r else "forward")
                seen.update(["position > 0"] * (p > 0) + ["variable < total"] * (v < m) + ["variable == total > 0"] * (v == m and m > 0))
        if any(a >= 0 and b < 0 for a, b in zip(first["index"], best["index"])):
            seen.add("tie")
    assert seen == {"first != best", "forward", "reverse", "position > 0", "variable < total", "variable == total > 0", "tie"}


def _counts_of(index, n_pool):
    index = np.asarray(index, dtype=np.int64)
    return np.bincount(index[index >= 0], minlength=n_pool)[:n_pool]


@pytest.mark.parametrize("case", ACCEPTED, ids=G.case_id)
def test_golden_indices_add_up_to_the_oracles_counts(oracle, case):
    for mode, use_first in (("first", True), ("best", False)):
        counts, total = oracle.count_single(case["reads"], case["template"], case["strand"], case["pool"], case["mismatches"], use_first)
        assert total == len(case["reads"])
        assert np.array_equal(_counts_of(case["expect"][mode]["index"], len(case["pool"])), counts), mode


@pytest.mark.parametrize("cell", A.CELLS, ids=A.IDS)
def test_edge_case_indices_add_up_to_the_oracles_counts(oracle, cell):
    """The reads of interest of every cell once (the batches repeat them)."""
    case = A.case(cell)
    assert all(len(b) == A.STAGE_BLOCK + 1 and b[-1] == b[-2] == i for i, b in enumerate(case.batches))
    assert max(len(r) for _, r, _, _ in case.items) == case.hint
    reads = [r for _, r, _, _ in case.items]
    for use_first in (True, False):
        counts, _ = oracle.count_single(reads, case.template, A.STRAND, case.pool, case.budget, use_first)
        index = case.expected(list(range(len(reads))), use_first)[0]
        assert np.array_equal(_counts_of(index, len(case.pool)), counts), use_first


def test_edge_cases_cover_every_outcome():
    """Across the cells: both strands, positions at and beyond 0, total and variable mismatches that differ and agree, reads
    that first mode assigns and best mode does not, and a best-mode match behind a tie."""
    seen = set()
    for cell in A.CELLS:
        for label, _, first, best in A.case(cell).items:
            for s in (first, best):
                if s[0] >= 0:
                    seen.add("reverse" if s[4] else "forward")
                    seen.update(["position > 0"] * (s[1] > 0) + ["variable < total"] * (s[3] < s[2]) + ["variable == total > 0"] * (s[3] == s[2] > 0))
            if first[0] >= 0 and best[0] < 0:
                seen.add("tie")
            if first != best and best[0] >= 0:
                seen.add("best elsewhere")
            if label == "tie-then-better" and best[1] > first[1]:
                seen.add("better after a tie")
    assert seen == {"forward", "reverse", "position > 0", "variable < total", "variable == total > 0", "tie", "best elsewhere", "better after a tie"}
