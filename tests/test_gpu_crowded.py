"""The library matcher (index_search, index_match, index_neighbours, pair_match) on crowded pools and on budgets above 3.

The pools of tests/gen.py::crowded_* hold entries one and two substitutions apart, at the edges of the index's position
groups and of the 64-bit words of the key planes; the queries are built for ties, unique hits at every distance up to the cap,
misses one substitution beyond it (tests/test_crowded_cpu.py checks that they are).  Budgets of 4 and 5 build no tables: the
dense node scans of all three key widths, the dense pair list of narrow keys and the seedless constant-region scan run.
Reads with substitutions in their flanks query an index built for the whole budget with a smaller cap.

Bit-exact against real kaori (tests/golden/kaori_crowded.json) for matchBarcodes, single and combinatorial counting -- and
a brute force for matchBarcodes; against the cache-free oracle for the paired-end and two-region entry points, where the
reference's own search cache depends on the order of the reads on exactly such pools."""
import functools

import numpy as np
import pytest

from tests import gen
from tests import golden_util as G
from tests.test_crowded_cpu import DUAL_CELLS, MATCH_NAMES, brute_match

pytestmark = pytest.mark.gpu

NAMES = list(gen.crowded_golden_cases())


@pytest.fixture(params=["staged", "general"])
def engine(request, monkeypatch):
    """The LDS-staged kernels and the byte-wise general engine (as tests/test_gpu_parity.py)."""
    if request.param == "general":
        monkeypatch.setenv("SCG_FORCE_GENERAL", "1")
    else:
        monkeypatch.delenv("SCG_FORCE_GENERAL", raising=False)
    return request.param


_reference = {}


def reference(key, compute):
    """The oracle's answer for a case, computed once for all the tests that compare with it."""
    if key not in _reference:
        _reference[key] = compute()
    return _reference[key]


@pytest.mark.parametrize("name", MATCH_NAMES)
def test_match(sc, gpu, name):
    """matchBarcodes: lengths 8..256 (narrow, wide and big keys, at and around their word edges) x budgets 0..5 x reverse."""
    case, expect = G.crowded(name)
    idx, mm = sc.match_barcodes(case["sequences"], case["choices"], case["substitutions"], case["reverse"])
    brute = brute_match(case["choices"], case["sequences"], case["substitutions"], case["reverse"])
    assert np.array_equal(idx, brute[0]) and np.array_equal(mm, brute[1])
    assert idx.tolist() == expect["index"] and mm.tolist() == expect["mismatches"]


@pytest.mark.parametrize("name", [n for n in NAMES if n.startswith("single-")])
def test_single(sc, gpu, engine, name):
    """countSingleBarcodes: lengths 20, 40, 100 x budgets 1..4 x first / best, both strands, caps of 0..budget."""
    case, expect = G.crowded(name)
    seqs, offs = sc.upload_reads(case["reads"], gpu)
    with sc.Plan.single(case["template"], case["strand"], case["pool"], case["mismatches"], case["use_first"]) as plan:
        plan.count(seqs, offs)
        counts, total = plan.read()
    assert total == expect["total"] and counts.tolist() == expect["counts"]
    assert sum(expect["counts"]) > len(case["reads"]) // 4


@pytest.mark.parametrize("grid", ["dense", "sparse"])
@pytest.mark.parametrize("name", [n for n in NAMES if n.startswith("combo-")])
def test_combo(sc, gpu, engine, name, grid, monkeypatch):
    """countComboBarcodes: regions of (12, 10) and (40, 8) bases x budgets 2 and 4, one budget shared in order; as a dense
    histogram and through the sorted key streams (as tests/test_gpu_sparse.py)."""
    if grid == "sparse":
        monkeypatch.setenv("SCG_DENSE_CELLS", "0")
    case, expect = G.crowded(name)
    seqs, offs = sc.upload_reads(case["reads"], gpu)
    with sc.Plan.combo(case["template"], case["strand"], case["pool0"], case["pool1"], case["mismatches"], case["use_first"]) as plan:
        plan.count(seqs, offs)
        idx, freq, total = plan.read_combo()
    assert total == expect["total"]
    assert np.array_equal(idx, np.asarray(expect["indices"], dtype=np.int32).reshape(2, -1)) and freq.tolist() == expect["freq"]
    assert sum(expect["freq"]) > len(case["reads"]) // 4


@functools.lru_cache(maxsize=None)
def dual_case(lens, budgets, randomized):
    return gen.crowded_dual_case(gen.CROWDED_SEED, lens, budgets, randomized, True)


def dual_args(c, use_first, distinct=False):
    pool1, pool2 = (list(dict.fromkeys(c[k])) for k in ("pool1", "pool2")) if distinct else (c["pool1"], c["pool2"])
    return (c["template1"], c["reverse1"], c["mismatches1"], pool1, c["template2"], c["reverse2"], c["mismatches2"], pool2,
            c["randomized"], use_first)


def paired(sc, gpu, c, make_plan, read):
    s1, o1 = sc.upload_reads(c["reads1"], gpu)
    s2, o2 = sc.upload_reads(c["reads2"], gpu)
    with make_plan() as plan:
        plan.count_paired(s1, s2, o1, o2)
        return getattr(plan, read)()


dual_cells = pytest.mark.parametrize("lens,budgets", DUAL_CELLS, ids=lambda v: "-".join(map(str, v)))
both = lambda name: pytest.mark.parametrize(name, [False, True], ids=lambda v: f"{name}={int(v)}")     # noqa: E731


@dual_cells
@both("randomized")
@both("use_first")
def test_dual(sc, oracle, gpu, engine, lens, budgets, randomized, use_first):
    """countDualBarcodes: keys of (12, 10), (40, 36), (100, 70) bases.  Mate 1's pool overflows pair_match's neighbour arrays
    near a centre (nested search), mate 2's never does (crossed arrays); budgets (4, 4) take the dense pair list (narrow) and
    the dense scans (wide).  Valid pairs: a strict subset with ties between two valid pairs and pairs with invalid partners only."""
    c = dual_case(lens, budgets, randomized)
    args = dual_args(c, use_first)
    exp = reference(("dual", lens, budgets, randomized, use_first), lambda: oracle.count_dual(c["reads1"], c["reads2"], *args))
    got = paired(sc, gpu, c, lambda: sc.Plan.dual(*args), "read")
    assert got[1] == exp[1] and np.array_equal(got[0], exp[0])
    assert len(c["reads1"]) // 8 < exp[0].sum() < len(c["reads1"])


@dual_cells
@both("randomized")
@both("use_first")
def test_dual_diagnostics(sc, oracle, gpu, engine, lens, budgets, randomized, use_first):
    """include.invalid=TRUE: each mate matched on its own (ties go to the first of the barcodes that recur over the rows),
    valid rows, invalid combinations and one-sided matches."""
    c = dual_case(lens, budgets, randomized)
    args = dual_args(c, use_first)
    exp = reference(("diag", lens, budgets, randomized, use_first), lambda: oracle.count_dual_diag(c["reads1"], c["reads2"], *args))
    got = paired(sc, gpu, c, lambda: sc.Plan.dual(*args, diagnostics=True), "read_diagnostics")
    for key in exp:
        assert np.array_equal(np.asarray(exp[key]), np.asarray(got[key])), key
    assert len(exp["freq"]) > 0 and exp["counts"].sum() > 0


@dual_cells
@both("randomized")
@both("use_first")
def test_paired_combo(sc, oracle, gpu, engine, lens, budgets, randomized, use_first):
    """countPairedComboBarcodes over the distinct barcodes of the same reads."""
    c = dual_case(lens, budgets, randomized)
    args = dual_args(c, use_first, distinct=True)
    exp = reference(("paired", lens, budgets, randomized, use_first), lambda: oracle.count_combo_paired(c["reads1"], c["reads2"], *args))
    got = paired(sc, gpu, c, lambda: sc.Plan.paired_combo(*args), "read_diagnostics")
    for key in exp:
        assert np.array_equal(np.asarray(exp[key]), np.asarray(got[key])), key
    assert len(exp["freq"]) > 0


@functools.lru_cache(maxsize=None)
def single_end_case(lens, budget):
    return gen.crowded_dual_single_end_case(gen.CROWDED_SEED, lens, budget)


single_end_cells = pytest.mark.parametrize("lens", [(12, 12), (20, 20), (50, 50)], ids=lambda v: f"key{sum(v)}")


@single_end_cells
@pytest.mark.parametrize("budget", [1, 3, 4])
def test_dual_single_end(sc, oracle, gpu, engine, lens, budget):
    """countDualBarcodesSingleEnd: combined keys of 24 (narrow), 40 (wide) and 100 (big) bases, the rows of a crowded pool."""
    c = single_end_case(lens, budget)
    args = (c["template"], c["strand"], c["pools"], c["mismatches"], c["use_first"])
    exp = reference(("single_end", lens, budget), lambda: oracle.count_dual_single_end(c["reads"], *args))
    seqs, offs = sc.upload_reads(c["reads"], gpu)
    with sc.Plan.dual_single_end(*args) as plan:
        plan.count(seqs, offs)
        got = plan.read()
    assert got[1] == exp[1] and np.array_equal(got[0], exp[0])
    assert len(c["reads"]) // 8 < exp[0].sum() < len(c["reads"])


@single_end_cells
@pytest.mark.parametrize("budget", [1, 3, 4])
def test_dual_single_end_diagnostics(sc, oracle, gpu, engine, lens, budget, tmp_path):
    """include.invalid=TRUE: the regions matched one by one, barcodes shared by several rows going to the first."""
    from oracle.pyoracle import write_fastq
    c = single_end_case(lens, budget)
    exp = reference(("single_end_diag", lens, budget), lambda: oracle.count_dual_single_end_diag(
        c["reads"], c["template"], c["strand"], c["pools"], c["mismatches"], c["use_first"]))
    fq = str(tmp_path / "x.fastq")
    write_fastq(fq, c["reads"])
    counts, (idx, freq), total = sc.count_dual_barcodes_single_end(fq, c["template"], c["pools"], c["strand"], c["mismatches"],
                                                                   c["use_first"], True, 1)
    assert total == exp["total"] and np.array_equal(counts, exp["counts"])
    assert np.array_equal(idx, exp["indices"]) and np.array_equal(freq, exp["freq"])
    assert exp["counts"].sum() > 0
