"""The restatement of the region-combination handler (tests/combo_regions_ref.py: constant mismatches in Python, the regions
looked up through the oracle's match_barcodes, find_match's walk, the first / best rule and the sort) against what the real
kaori::CombinatorialBarcodesSingleEnd<256, V> gave on the same inputs for V = 1, 2, 3, 4, 5 and 8
(tests/golden/kaori_combo_regions.json, written by tools/gen_combo_regions_golden.py): combinations, counts, totals and
the messages of the arguments the reference rejects, in both modes.  At V = 2 the restatement also has to agree with the
oracle's count_combo on seeded cases.  No GPU, nothing from a reference checkout."""
import random

import numpy as np
import pytest

from tests import combo_regions_ref as ref
from tests import gen
from tests import golden_util as G

CASES = G.load("kaori_combo_regions.json")


def test_goldens_cover_the_handler():
    accepted = [c for c in CASES if "error" not in c["expect"]["best"]]
    assert 50 <= len(CASES) <= 70 and 4 * (len(CASES) - len(accepted)) <= len(CASES) and len(accepted) < len(CASES)
    assert {len(c["pools"]) for c in accepted} == {1, 2, 3, 4, 5, 8}
    assert {c["strand"] for c in accepted} == {0, 1, 2} and {c["mismatches"] for c in accepted} == {0, 1, 2, 3}
    longest = [max(len(p[0]) for p in c["pools"]) for c in accepted]
    assert min(longest) <= 32 and any(32 < v <= 64 for v in longest) and max(longest) > 64
    assert any(c["template"].startswith("-") for c in accepted) and any(c["template"].endswith("-") for c in accepted)
    assert any(any(len(p) == 1 for p in c["pools"]) for c in accepted) and any(len({len(p) for p in c["pools"]}) > 1 for c in accepted)
    assert any(any(ch in gen.IUPAC for p in c["pools"] for s in p for ch in s) for c in accepted)
    assert any(c["expect"]["first"]["combinations"] != c["expect"]["best"]["combinations"] for c in accepted)
    assert all(c["expect"][m]["combinations"] for c in accepted for m in ("first", "best"))


@pytest.mark.parametrize("use_first", [True, False], ids=["first", "best"])
@pytest.mark.parametrize("case", CASES, ids=G.case_id)
def test_restatement_reproduces_kaori(oracle, case, use_first):
    from oracle.pyoracle import OracleError
    expect = case["expect"]["first" if use_first else "best"]
    args = (case["reads"], case["template"], case["strand"], case["pools"], case["mismatches"], use_first)
    if "error" in expect:
        with pytest.raises(OracleError) as e:
            ref.count_combo_regions(oracle, *args)
        assert str(e.value) == expect["error"]
        return
    idx, freq, total = ref.count_combo_regions(oracle, *args)
    assert total == expect["total"] == len(case["reads"])
    assert ref.indices_list(idx, freq) == expect["combinations"]


@pytest.mark.parametrize("seed", range(12))
def test_two_regions_equal_the_oracles_count_combo(oracle, seed):
    rng = random.Random(4100 + seed)
    c = gen.random_combo_case(rng, sizes=(30, 120), wide={0: False, 1: True, 2: "big"}[seed % 3])
    from oracle.pyoracle import OracleError
    for use_first in (True, False):
        theirs = (c["reads"], c["template"], c["strand"], c["pool0"], c["pool1"], c["mismatches"], use_first)
        mine = (c["reads"], c["template"], c["strand"], [c["pool0"], c["pool1"]], c["mismatches"], use_first)
        try:
            want = oracle.count_combo(*theirs)
        except OracleError as rejected:                       # (random IUPAC codes that expand to one sequence twice)
            with pytest.raises(OracleError) as e:
                ref.count_combo_regions(oracle, *mine)
            assert str(e.value) == str(rejected)
            continue
        got = ref.count_combo_regions(oracle, *mine)
        assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1]) and got[2] == want[2]
