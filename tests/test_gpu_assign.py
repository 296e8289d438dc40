"""Plan.assign / scg_assign_batch on the GPU: the match state of every read (index, position, mismatches,
variable_mismatches, reverse), exact against kaori::SimpleSingleMatch's own results (tests/golden/kaori_assign.json,
written by tools/gen_assign_golden.py) and against the constructed edge cases of tests/assign_cases.py (checked against
the reference by the same tool) in each of the 18 shapes of assign_staged_kernel, on the byte-wise assign_kernel, and
through every argument form of the entry."""
import gzip
import os
import random

import numpy as np
import pytest

from tests import assign_cases as A
from tests import gen
from tests import golden_util as G

pytestmark = pytest.mark.gpu

FIELDS = A.FIELDS
CASES = G.load("kaori_assign.json")
RAGGED = [c for c in CASES if c["group"] in ("short", "wide", "big")]
MODES = (("first", True), ("best", False))
WRONG_KIND = "scg_assign_batch needs a single-barcode plan (scg_plan_single)"


def _plan(sc, case, use_first):
    return sc.Plan.single(case["template"], case["strand"], case["pool"], case["mismatches"], use_first)


def _same(got, expect, what):
    """Exact equality of all five arrays with the lists (or arrays) expected."""
    for f, t, e in zip(FIELDS, got, expect):
        assert t.dtype == (np.int32 if f in ("index", "position") else np.int8), (what, f, t.dtype)
        bad = np.nonzero(t.astype(np.int64) != np.asarray(e, dtype=np.int64))[0]
        assert bad.size == 0, (what, f, bad[:5].tolist(), t[bad[:5]].tolist(), np.asarray(e)[bad[:5]].tolist())


def _host(assignment):
    return [None if t is None else t.cpu().numpy() for t in assignment]


def _golden(case, mode):
    return [case["expect"][mode][f] for f in FIELDS]


@pytest.mark.parametrize("engine", ["staged", "general"])
@pytest.mark.parametrize("case", RAGGED, ids=G.case_id)
def test_golden_cases_as_ragged_batches(sc, gpu, case, engine, monkeypatch):
    """Keys of up to 64 bases take assign_staged_kernel, the 65-120-base group assign_kernel<Big>; SCG_FORCE_GENERAL=1 sends
    every case through assign_kernel."""
    if engine == "general":
        monkeypatch.setenv("SCG_FORCE_GENERAL", "1")
    for mode, use_first in MODES:
        if "error" in case["expect"][mode]:
            with pytest.raises(sc.ScgError) as e:
                _plan(sc, case, use_first)
            assert str(e.value) == case["expect"][mode]["error"]
            continue
        seqs, offs = sc.upload_reads(case["reads"], gpu)
        with _plan(sc, case, use_first) as plan:
            got = plan.assign(seqs, offs)
            assert all(t.device == seqs.device and t.shape == (len(case["reads"]),) for t in got)
            _same(_host(got), _golden(case, mode), (case["source"], mode, engine))
            counts, total = plan.read()          # (assigning counts nothing)
            assert total == 0 and not counts.any()


@pytest.mark.parametrize("cell", A.CELLS, ids=A.IDS)
def test_every_staged_shape_at_its_tile_edges(sc, gpu, cell):
    """Each batch once with the cell's max_len hint and once with max_len=0, where the binding computes it."""
    case = A.case(cell)
    for mode, use_first in MODES:
        with sc.Plan.single(case.template, A.STRAND, case.pool, case.budget, use_first) as plan:
            for batch in case.batches:
                seqs, offs = sc.upload_reads(case.reads(batch), gpu)
                expect = case.expected(batch, use_first)
                for hint in (case.hint, 0):
                    got = _host(plan.assign(seqs, offs, max_len=hint))
                    _same(got, expect, (cell["id"], mode, case.items[batch[-1]][0], hint))
            counts, total = plan.read()          # (also: no lane flagged its read as unstaged)
            assert total == 0 and not counts.any()


@pytest.mark.parametrize("case", [c for c in CASES if c["group"] == "fixed"], ids=G.case_id)
def test_fixed_length_batches(sc, gpu, case):
    import torch
    L = case["fixed_len"]
    seqs = torch.from_numpy(np.frombuffer("".join(case["reads"]).encode(), dtype=np.uint8).copy()).to(gpu)
    for mode, use_first in MODES:
        if "error" in case["expect"][mode]:
            with pytest.raises(sc.ScgError):
                _plan(sc, case, use_first)
            continue
        with _plan(sc, case, use_first) as plan:
            _same(_host(plan.assign(seqs, fixed_len=L)), _golden(case, mode), (case["source"], mode))
            head = plan.assign(seqs, fixed_len=L, n_reads=7)
            _same(_host(head), [x[:7] for x in _golden(case, mode)], (case["source"], mode, "n_reads=7"))


@pytest.mark.parametrize("case", [c for c in CASES if c["group"] == "long"], ids=G.case_id)
def test_long_reads_take_the_general_kernel(sc, gpu, case):
    assert max(len(r) for r in case["reads"]) >= 321
    seqs, offs = sc.upload_reads(case["reads"], gpu)
    for mode, use_first in MODES:
        if "error" in case["expect"][mode]:
            with pytest.raises(sc.ScgError):
                _plan(sc, case, use_first)
            continue
        with _plan(sc, case, use_first) as plan:
            _same(_host(plan.assign(seqs, offs)), _golden(case, mode), (case["source"], mode))


@pytest.fixture(scope="module")
def workload():
    """5 000 reads of one template and pool, both strands (shared; never modified)."""
    rng = random.Random(4)
    template = gen.make_template(rng, 1, [14], 6, 10)
    pool = gen.make_pool(rng, 40, 14, gen.BASES, min_dist=2)
    reads = gen.make_reads(rng, template, [pool], 5000, 2, 0.03, 0.01, 0.1, 0.1, 30)
    return dict(template=template, pool=pool, reads=reads, strand=2, mismatches=2)


@pytest.mark.parametrize("mode,use_first", MODES)
def test_counting_and_assigning_interleave_on_one_plan(sc, oracle, gpu, workload, mode, use_first):
    w = workload
    expect, total = oracle.count_single(w["reads"], w["template"], w["strand"], w["pool"], w["mismatches"], use_first)
    seqs, offs = sc.upload_reads(w["reads"], gpu)
    with sc.Plan.single(w["template"], w["strand"], w["pool"], w["mismatches"], use_first) as plan:
        plan.count(seqs, offs)
        got = plan.assign(seqs, offs)
        plan.count(seqs, offs)
        counts, n = plan.read()
        assert n == 2 * len(w["reads"]) == 2 * total and np.array_equal(counts, 2 * expect)
        index = got.index.cpu().numpy().astype(np.int64)
        assert np.array_equal(np.bincount(index[index >= 0], minlength=len(w["pool"])), expect)
        only = plan.assign(seqs, offs, fields=("index",))
        assert only.position is None and only.mismatches is None and only.variable_mismatches is None and only.reverse is None
        assert np.array_equal(only.index.cpu().numpy(), index)
        some = plan.assign(seqs, offs, fields=("reverse", "index"))
        assert some.position is None and np.array_equal(some.reverse.cpu().numpy(), got.reverse.cpu().numpy())
        assert plan.read()[1] == 2 * len(w["reads"])
        with pytest.raises(ValueError):
            plan.assign(seqs, offs, fields=("position",))


def test_non_default_stream(sc, gpu):
    import torch
    case = next(c for c in RAGGED if "error" not in c["expect"]["best"] and len(c["reads"]) >= 30)
    seqs, offs = sc.upload_reads(case["reads"], gpu)
    torch.cuda.synchronize()
    stream = torch.cuda.Stream(device=gpu)
    with _plan(sc, case, False) as plan:
        got = plan.assign(seqs, offs, stream=stream)
        stream.synchronize()
        _same(_host(got), _golden(case, "best"), case["source"])


def test_other_plan_kinds_are_refused(sc, gpu):
    from screencounter_amd import _lib
    seqs, offs = sc.upload_reads(["ACGTAAAATGCA"], gpu)
    P = sc.Plan
    plans = {
        "combo": lambda: P.combo("ACGT----TG--CA", 2, ["AAAA"], ["CC"]),
        "dual": lambda: P.dual("AC--GT", False, 0, ["AA"], "AC--GT", False, 0, ["CC"]),
        "single_paired": lambda: P.single_paired("ACGT----TGCA", 2, ["AAAA"]),
        "dual_single_end": lambda: P.dual_single_end("ACGT----TG--CA", 2, [["AAAA"], ["CC"]]),
        "dual_single_end, one region": lambda: P.dual_single_end("ACGT----TGCA", 2, [["AAAA"]]),
        "paired_combo": lambda: P.paired_combo("AC--GT", False, 0, ["AA"], "AC--GT", False, 0, ["CC"]),
        "random": lambda: P.random("ACGT----TGCA", 2),
    }
    for name, make in plans.items():
        with make() as plan:
            with pytest.raises(sc.ScgError) as e:
                plan.assign(seqs, offs)
            assert e.value.code == _lib.SCG_ERR_INVALID and str(e.value) == WRONG_KIND, name
    with P.single("ACGT----TGCA", 2, ["AAAA"]) as plan:
        L, err = sc.load(), _lib.errbuf()
        rc = L.scg_assign_batch(plan._h, seqs.data_ptr(), offs.data_ptr(), 0, 12, 1, None, None, None, None, None, None, err, _lib.ERRCAP)
        assert rc == _lib.SCG_ERR_INVALID and err.value == b"null argument"
    with P.single("ACGT" + "-" * 200 + "TGCA", 2, ["A" * 200], 128) as plan:
        with pytest.raises(sc.ScgError) as e:
            plan.assign(seqs, offs)
        assert e.value.code == _lib.SCG_ERR_UNSUPPORTED and "127" in str(e.value)


def test_empty_batch(sc, gpu):
    import torch
    seqs, offs = sc.upload_reads([], gpu)
    with sc.Plan.single("ACGT----TGCA", 2, ["AAAA"]) as plan:
        got = plan.assign(seqs, offs)
        assert all(t.shape == (0,) for t in got)
        assert got.index.dtype == torch.int32 and got.position.dtype == torch.int32
        assert {got.mismatches.dtype, got.variable_mismatches.dtype, got.reverse.dtype} == {torch.int8}
        assert plan.read()[1] == 0


def test_max_len_declared_too_small_is_reported_by_read(sc, gpu):
    """The handled error flag: the staged kernel does not search a read that does not fit its tile, and says so."""
    reads = ["ACGTAAAATGCA" + "T" * 30, "ACGTAAAATGCA" + "G" * 200]
    seqs, offs = sc.upload_reads(reads, gpu)
    with sc.Plan.single("ACGT----TGCA", 2, ["AAAA"]) as plan:
        got = plan.assign(seqs, offs, max_len=100)
        assert got.index.cpu().tolist() == [0, -1] and got.position.cpu().tolist() == [0, -1]
        with pytest.raises(sc.ScgError, match="a read is longer than the max_len declared for its batch"):
            plan.read()


@pytest.mark.parametrize("gz", [False, True], ids=["plain", "gzip"])
def test_assign_single_barcodes_over_a_file(sc, gpu, tmp_path, gz):
    case = next(c for c in RAGGED if "error" not in c["expect"]["best"] and len(c["reads"]) >= 30)
    path = os.path.join(str(tmp_path), "reads.fastq" + (".gz" if gz else ""))
    with (gzip.open if gz else open)(path, "wb") as f:
        f.write(gen.fastq_text(case["reads"]))
    for mode, use_first in MODES:
        got = sc.assign_single_barcodes(path, case["template"], case["strand"], case["pool"], case["mismatches"], use_first, batch_reads=7)
        assert type(got).__name__ == "Assignment" and all(isinstance(t, np.ndarray) for t in got)
        _same(list(got), _golden(case, mode), (case["source"], mode, gz))
