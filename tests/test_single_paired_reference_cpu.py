"""The composed reference of the paired single-barcode handler (tests/single_paired_ref.py: the single-end oracle on one
read at a time plus the rule of SingleBarcodePairedEnd.hpp:93-122) against what the real kaori::SingleBarcodePairedEnd
gave on the same inputs (tests/golden/kaori_single_paired.json, written by tools/gen_single_paired_golden.py): counts,
totals and the messages of the pools the reference rejects, in both modes."""
import numpy as np
import pytest

from tests import golden_util as G
from tests import single_paired_ref as ref

CASES = G.load("kaori_single_paired.json")


def test_goldens_cover_the_rule():
    assert len(CASES) >= 35 and all(len(c["reads1"]) == len(c["reads2"]) <= 60 for c in CASES)
    assert {c["strand"] for c in CASES} == {0, 1, 2} and {c["mismatches"] for c in CASES} == {0, 1, 2, 3}
    lengths = {len(c["pool"][0]) for c in CASES}
    assert any(n <= 32 for n in lengths) and any(33 <= n <= 64 for n in lengths) and any(65 <= n <= 120 for n in lengths)
    assert any("error" in c["expect"]["best"] for c in CASES)
    assert any(c["expect"]["first"].get("counts") != c["expect"]["best"].get("counts") for c in CASES)


@pytest.mark.parametrize("use_first", [True, False], ids=["first", "best"])
@pytest.mark.parametrize("case", CASES, ids=G.case_id)
def test_composed_reference_reproduces_kaori(oracle, case, use_first):
    from oracle.pyoracle import OracleError
    expect = case["expect"]["first" if use_first else "best"]
    args = (case["reads1"], case["reads2"], case["template"], case["strand"], case["pool"], case["mismatches"], use_first)
    if "error" in expect:
        with pytest.raises(OracleError) as e:
            ref.count_single_paired(oracle, *args)
        assert str(e.value) == expect["error"]
        return
    counts, total = ref.count_single_paired(oracle, *args)
    assert total == expect["total"] == len(case["reads1"])
    assert np.array_equal(counts, np.asarray(expect["counts"], dtype=np.int32))
