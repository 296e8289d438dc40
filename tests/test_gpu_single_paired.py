"""One barcode on either mate of a pair (kaori::SingleBarcodePairedEnd, handlers/SingleBarcodePairedEnd.hpp:93-124) on the
GPU: Plan.single_paired on uploaded mates and the two file entries, staged and byte-wise (SCG_FORCE_GENERAL=1), against

  - the real handler's outputs (tests/golden/kaori_single_paired.json), and
  - the composed reference (tests/single_paired_ref.py: the single-end oracle on one read at a time plus the handler's
    rule), which test_single_paired_reference_cpu.py pins to those goldens.

The composed reference costs about 1.4 ms per pair; every test here keeps to 1 500 pairs or fewer, and batches that
repeat a few kinds of pair ask it once per kind (PairRef)."""
import gzip
import random

import numpy as np
import pytest

from tests import gen
from tests import golden_util as G
from tests import single_paired_ref as ref

pytestmark = pytest.mark.gpu

GOLDENS = G.load("kaori_single_paired.json")
MODES = ((True, "first"), (False, "best"))


@pytest.fixture(params=["staged", "general"])
def engine(request, monkeypatch):
    if request.param == "general":
        monkeypatch.setenv("SCG_FORCE_GENERAL", "1")
    return request.param


class PairRef:
    """The composed reference with one question per distinct (mate 1, mate 2)."""

    def __init__(self, oracle, template, strand, pool, mismatches):
        self.oracle, self.args, self.n_pool, self.seen = oracle, (template, strand, pool, mismatches), len(pool), {}

    def index(self, a, b, use_first):
        key = (a, b, use_first)
        if key not in self.seen:
            self.seen[key] = ref.pair_index(self.oracle, a, b, *self.args, use_first)
        return self.seen[key]

    def counts(self, reads1, reads2, use_first):
        out = np.zeros(self.n_pool, dtype=np.int32)
        for a, b in zip(reads1, reads2):
            i = self.index(a, b, use_first)
            if i >= 0:
                out[i] += 1
        return out


def upload(sc, reads, fixed):
    """Arguments of one mate for count_paired: (seqs, offsets, fixed_len)."""
    seqs, offs = sc.upload_reads(reads, "cuda:0")
    if not fixed:
        return seqs, offs, 0
    assert len({len(r) for r in reads}) == 1 and len(reads[0]) > 0
    return seqs, None, len(reads[0])


def count_plan(sc, plan, reads1, reads2, fixed=(False, False)):
    s1, o1, f1 = upload(sc, reads1, fixed[0])
    s2, o2, f2 = upload(sc, reads2, fixed[1])
    plan.count_paired(s1, s2, o1, o2, fixed_len1=f1, fixed_len2=f2, n_pairs=len(reads1))


def run_plan(sc, template, strand, pool, mismatches, use_first, reads1, reads2, fixed=(False, False)):
    with sc.Plan.single_paired(template, strand, pool, mismatches, use_first, device=0) as plan:
        count_plan(sc, plan, reads1, reads2, fixed)
        counts, total = plan.read()
    return counts[:len(pool)], total


def write_mates(tmp_path, reads1, reads2, form="plain", stem="m"):
    paths = []
    for k, reads in enumerate((reads1, reads2)):
        text = gen.fastq_text(reads)
        if form == "plain":
            p = tmp_path / f"{stem}{k + 1}.fastq"
            p.write_bytes(text)
        elif form == "bgzf":
            p = tmp_path / f"{stem}{k + 1}.bgzf.gz"
            gen.write_bgzf(str(p), text, block=3000)
        else:
            p = tmp_path / f"{stem}{k + 1}.fastq.gz"
            with gzip.open(p, "wb") as f:
                f.write(text)
        paths.append(str(p))
    return paths


# ---- goldens -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", GOLDENS, ids=G.case_id)
def test_goldens_through_the_plan(sc, gpu, engine, case):
    from screencounter_amd import _lib
    for use_first, mode in MODES:
        expect = case["expect"][mode]
        args = (case["template"], case["strand"], case["pool"], case["mismatches"], use_first)
        if "error" in expect:
            with pytest.raises(sc.ScgError) as e:
                run_plan(sc, *args, case["reads1"], case["reads2"])
            assert (e.value.code, str(e.value)) == (_lib.SCG_ERR_INVALID, expect["error"])
            continue
        counts, total = run_plan(sc, *args, case["reads1"], case["reads2"])
        assert total == expect["total"], mode
        assert np.array_equal(counts, np.asarray(expect["counts"], dtype=np.int32)), mode


@pytest.mark.parametrize("case", GOLDENS, ids=G.case_id)
def test_goldens_through_the_file_entry(sc, gpu, engine, tmp_path, case):
    from screencounter_amd import _lib
    for form in ("plain", "gzip"):
        p1, p2 = write_mates(tmp_path, case["reads1"], case["reads2"], form)
        for use_first, mode in MODES:
            expect = case["expect"][mode]
            args = (p1, p2, case["template"], case["strand"], case["pool"], case["mismatches"], use_first)
            if "error" in expect:
                with pytest.raises(sc.ScgError) as e:
                    sc.count_single_barcodes_paired(*args)
                assert (e.value.code, str(e.value)) == (_lib.SCG_ERR_INVALID, expect["error"])
                continue
            counts, total = sc.count_single_barcodes_paired(*args)
            assert total == expect["total"], (form, mode)
            assert np.array_equal(counts, np.asarray(expect["counts"], dtype=np.int32)), (form, mode)


# ---- random parity -------------------------------------------------------------------------------------------------------
# (seed, keyword arguments of gen.random_single_case, cases): narrow, wide and big keys; the seeds' cases cover the three
# strands and the budgets 0-3 (asserted below)
RANDOM_GROUPS = [(101, dict(max_vlen=32), 10), (102, dict(min_vlen=33, max_vlen=64), 6), (103, dict(min_vlen=65, max_vlen=240), 6)]
_random_cases = {}


def random_cases(oracle):
    """The seeded cases with the composed reference's answer in both modes, computed once for both engines."""
    from oracle.pyoracle import OracleError
    if not _random_cases:
        cases = []
        for seed, kwargs, n in RANDOM_GROUPS:
            rng = random.Random(seed)
            for _ in range(n):
                c = ref.paired_case(rng, sizes=(1, 30, 60), **kwargs)
                c["expect"] = {}
                for use_first, mode in MODES:
                    try:
                        counts, total = ref.count_single_paired(oracle, c["reads1"], c["reads2"], c["template"], c["strand"], c["pool"],
                                                                c["mismatches"], use_first)
                        c["expect"][mode] = (counts, total)
                    except OracleError as e:
                        c["expect"][mode] = str(e)
                cases.append(c)
        _random_cases["cases"] = cases
    return _random_cases["cases"]


def test_random_parity(sc, oracle, gpu, engine):
    from screencounter_amd import _lib
    cases = random_cases(oracle)
    assert sum(len(c["reads1"]) for c in cases) <= 1500
    assert {c["strand"] for c in cases} == {0, 1, 2} and {c["mismatches"] for c in cases} == {0, 1, 2, 3}
    assert any(len(c["pool"][0]) > 64 for c in cases) and any(32 < len(c["pool"][0]) <= 64 for c in cases)
    for k, c in enumerate(cases):
        for use_first, mode in MODES:
            args = (c["template"], c["strand"], c["pool"], c["mismatches"], use_first)
            expect = c["expect"][mode]
            if isinstance(expect, str):
                with pytest.raises(sc.ScgError) as e:
                    run_plan(sc, *args, c["reads1"], c["reads2"])
                assert (e.value.code, str(e.value)) == (_lib.SCG_ERR_INVALID, expect), k
                continue
            counts, total = run_plan(sc, *args, c["reads1"], c["reads2"])
            assert total == expect[1] and np.array_equal(counts, expect[0]), (k, mode, c["template"], c["strand"], c["mismatches"])


# ---- the rule, branch by branch ------------------------------------------------------------------------------------------
LEFT, RIGHT = "ACGTACGA", "TGCATGCA"
TEMPLATE = LEFT + "-" * 8 + RIGHT
# pairwise distances: 0-1 = 8, 0-2 = 8, 1-2 = 8, 2-3 = 2 (barcode 3 is barcode 2 with its first two bases changed)
POOL4 = ["AAAAAAAA", "CCCCCCCC", "GGGGGGGG", "TTGGGGGG"]


def construct(barcode):
    """A read with the barcode's construct: bases 2-9 the left flank, 10-17 the barcode, 18-25 the right flank."""
    return "TT" + LEFT + barcode + RIGHT + "AC"


def sub(s, *positions):
    """s with the bases at `positions` replaced by another base."""
    out = list(s)
    for p in positions:
        out[p] = "C" if out[p] != "C" else "A"
    return "".join(out)


JUNK = "TTTTTTTTTTTTTTTTTTTTTTTTTTTTTT"


def rule_batch():
    """(name, mate 1, mate 2, index in first mode, index in best mode) at budget 2."""
    b = [construct(x) for x in POOL4]
    ambiguous = construct("TGGGGGGG")          # one substitution from barcode 2 and one from barcode 3
    return [
        ("mate 1 only", b[0], JUNK, 0, 0),
        ("mate 2 only", JUNK, b[1], 1, 1),
        ("mate 1 fewer mismatches", b[0], sub(b[1], 3), 0, 0),
        ("mate 2 fewer mismatches", sub(b[0], 3, 20), sub(b[1], 12), 0, 1),
        ("equal mismatches, same barcode", sub(b[1], 2), sub(b[1], 25), 1, 1),
        ("equal mismatches, different barcodes", sub(b[0], 5), sub(b[1], 13), 0, -1),
        ("mate 1 ambiguous, mate 2 clean", ambiguous, b[0], 0, 0),
        ("mate 2 ambiguous, mate 1 one mismatch", sub(b[1], 3), ambiguous, 1, 1),
        ("neither mate", JUNK, JUNK[:-3], -1, -1),
    ]


def test_the_rule_branch_by_branch(sc, oracle, gpu, engine):
    batch = rule_batch()
    pair_ref = PairRef(oracle, TEMPLATE, 0, POOL4, 2)
    reads1, reads2 = [r[1] for r in batch], [r[2] for r in batch]
    for use_first, mode in MODES:
        want = [r[3] if use_first else r[4] for r in batch]
        # the expectations written from the rule are the composed reference's
        assert [pair_ref.index(a, b, use_first) for a, b in zip(reads1, reads2)] == want, mode
        expect = np.bincount([i for i in want if i >= 0], minlength=len(POOL4))
        counts, total = run_plan(sc, TEMPLATE, 0, POOL4, 2, use_first, reads1, reads2)
        assert total == len(batch) and np.array_equal(counts, expect), (mode, counts, expect)
        # pair by pair, so that a failure names its branch
        for name, a, b, *_ in batch:
            counts, _ = run_plan(sc, TEMPLATE, 0, POOL4, 2, use_first, [a], [b])
            i = pair_ref.index(a, b, use_first)
            assert np.array_equal(counts, np.bincount([i] if i >= 0 else [], minlength=len(POOL4))), (mode, name)


# ---- tile and barrier edges ----------------------------------------------------------------------------------------------
EDGE_POOL = ["AAAAAAAA", "CCCCCCCC", "GGGGGGGG", "TTTTGGGG", "ACACACAC", "GTGTGTGT"]


def pad_to(read, n, filler="T"):
    assert len(read) <= n
    return read + filler * (n - len(read))


def edge_kinds(rng, template, pool, n1, n2, ragged1, ragged2):
    """A few kinds of pair for mates of n1 / n2 bases (ragged: up to that; the first pair has a mate of exactly that length):
    hits on mate 1, on mate 2, on both (equal and unequal mismatches), on neither, at the start and at the end of a read."""
    t = len(template)

    def mate(n, ragged, barcode, at_end=False, muts=()):
        if barcode is None:
            body = ""
        else:
            body = sub(gen.fill_template(template, [barcode]), *muts)
        if n < len(body):
            body = ""                                  # the mate is too short for the construct: it carries nothing
        length = n if not ragged else rng.randint(len(body), n)
        free = length - len(body)
        lead = free if at_end else rng.randint(0, free)
        return "T" * lead + body + "G" * (free - lead)

    kinds = []
    for i, (x, y, mx, my, end) in enumerate([(0, None, (), (), False), (None, 1, (), (), True), (2, 3, (1,), (), False), (4, 4, (2,), (t - 2,), True),
                                             (5, 0, (0,), (t - 1,), False), (None, None, (), (), False), (1, 2, (), (3,), True)]):
        kinds.append((mate(n1, ragged1 and i > 0, pool[x] if x is not None else None, end, mx),
                      mate(n2, ragged2 and i > 0, pool[y] if y is not None else None, not end, my)))
    return kinds


def check_batch(sc, pair_ref, template, strand, pool, mismatches, reads1, reads2, fixed=(False, False), what=None):
    for use_first, mode in MODES:
        counts, total = run_plan(sc, template, strand, pool, mismatches, use_first, reads1, reads2, fixed)
        expect = pair_ref.counts(reads1, reads2, use_first)
        assert total == len(reads1), (what, mode)
        assert np.array_equal(counts, expect), (what, mode, counts, expect)


@pytest.mark.parametrize("n_pairs", [1, 255, 256, 257, 513])
def test_partial_and_full_tiles(sc, oracle, gpu, engine, n_pairs):
    """The last workgroup's idle lanes go through both passes' barriers; fixed/fixed, fixed/ragged and ragged/ragged mates."""
    rng = random.Random(n_pairs)
    pair_ref = PairRef(oracle, TEMPLATE, 2, EDGE_POOL, 1)
    for ragged1, ragged2 in ((False, False), (False, True), (True, True)):
        kinds = edge_kinds(rng, TEMPLATE, EDGE_POOL, 60, 47, ragged1, ragged2)
        picks = [kinds[(7 * i + i // 5) % len(kinds)] for i in range(n_pairs)]
        picks = [(gen.rc(a), gen.rc(b)) if i % 3 == 0 else (a, b) for i, (a, b) in enumerate(picks)]
        reads1, reads2 = [p[0] for p in picks], [p[1] for p in picks]
        check_batch(sc, pair_ref, TEMPLATE, 2, EDGE_POOL, 1, reads1, reads2, (not ragged1, not ragged2), (ragged1, ragged2))


@pytest.mark.parametrize("where", ["all on mate 1", "all only on mate 2", "nowhere"])
def test_uniform_batches(sc, oracle, gpu, engine, where):
    """Every lane of every wavefront takes the same way through the second pass."""
    n = 300
    hit = [construct(EDGE_POOL[i % len(EDGE_POOL)]) for i in range(n)]
    miss = [JUNK] * n
    reads1, reads2 = {"all on mate 1": (hit, hit[::-1]), "all only on mate 2": (miss, hit), "nowhere": (miss, miss)}[where]
    pair_ref = PairRef(oracle, TEMPLATE, 0, EDGE_POOL, 1)
    check_batch(sc, pair_ref, TEMPLATE, 0, EDGE_POOL, 1, reads1, reads2, (True, True), where)
    counts, _ = run_plan(sc, TEMPLATE, 0, EDGE_POOL, 1, True, reads1, reads2, (True, True))
    assert int(counts.sum()) == (0 if where == "nowhere" else n)


def test_short_and_empty_mates(sc, oracle, gpu, engine):
    """A mate shorter than the template, or empty, counts as the other mate alone -- in the middle of a tile, at its ends and
    as a whole batch."""
    t = len(TEMPLATE)
    full = [construct(b) for b in EDGE_POOL]
    stubs = ["", "A", TEMPLATE.replace("-", "A")[:t - 1], LEFT]
    pair_ref = PairRef(oracle, TEMPLATE, 2, EDGE_POOL, 1)
    reads1, reads2 = [], []
    for i in range(290):
        a, b = full[i % len(full)], stubs[i % len(stubs)]
        if i % 3 == 1:
            a, b = b, gen.rc(a)
        elif i % 3 == 2:
            a, b = stubs[(i + 1) % len(stubs)], b
        reads1.append(a)
        reads2.append(b)
    reads1[0], reads2[0], reads1[-1], reads2[-1] = "", full[0], full[1], ""
    check_batch(sc, pair_ref, TEMPLATE, 2, EDGE_POOL, 1, reads1, reads2, what="mixed")
    expect_first = pair_ref.counts(reads1, reads2, True)
    assert int(expect_first.sum()) == sum(1 for a, b in zip(reads1, reads2) if len(a) >= t or len(b) >= t)
    # one mate empty throughout (a buffer of no bytes at all), the other carrying every construct
    check_batch(sc, pair_ref, TEMPLATE, 2, EDGE_POOL, 1, [""] * 40, (full * 7)[:40], what="mate 1 empty")
    check_batch(sc, pair_ref, TEMPLATE, 2, EDGE_POOL, 1, (full * 7)[:40], [""] * 40, what="mate 2 empty")


@pytest.mark.parametrize("lengths", [(150, 150), (150, 170), (161, 320), (96, 40), (320, 321)], ids=lambda x: f"{x[0]}x{x[1]}")
def test_mate_lengths_across_the_tile_shapes(sc, oracle, gpu, engine, lengths):
    """The longer mate picks the tile: 160 bases and fewer, 161-320, and beyond that the byte-wise kernel."""
    rng = random.Random(str(lengths))
    n1, n2 = lengths
    pair_ref = PairRef(oracle, TEMPLATE, 2, EDGE_POOL, 1)
    for ragged in (False, True):
        kinds = edge_kinds(rng, TEMPLATE, EDGE_POOL, n1, n2, ragged, ragged)
        picks = [kinds[(3 * i + i // 7) % len(kinds)] for i in range(270)]
        reads1, reads2 = [p[0] for p in picks], [p[1] for p in picks]
        assert max(map(len, reads1)) == n1 and max(map(len, reads2)) == n2
        check_batch(sc, pair_ref, TEMPLATE, 2, EDGE_POOL, 1, reads1, reads2, (not ragged, not ragged), ragged)


@pytest.mark.parametrize("flank", [(30, 30), (70, 70)], ids=["template of 68", "template of 148"])
def test_long_templates(sc, oracle, gpu, engine, flank):
    """Templates of more than 64 and more than 128 bases: four and eight plane words per window."""
    rng = random.Random(flank[0])
    template = gen.rand_seq(rng, flank[0]) + "-" * 8 + gen.rand_seq(rng, flank[1])
    pair_ref = PairRef(oracle, template, 2, EDGE_POOL, 2)
    for n1, n2 in ((160, 152), (200, 310)):
        kinds = edge_kinds(rng, template, EDGE_POOL, n1, n2, False, True)
        picks = [kinds[(5 * i + i // 3) % len(kinds)] for i in range(260)]
        check_batch(sc, pair_ref, template, 2, EDGE_POOL, 2, [p[0] for p in picks], [p[1] for p in picks], (True, False), (n1, n2))


@pytest.mark.parametrize("max_len", [119, 120], ids=["96 positions", "97 positions"])
def test_compact_and_full_candidate_masks(sc, oracle, gpu, engine, max_len):
    """max_len - template + 1 <= 96 takes the three-word candidate mask, one base more the full one; the longer mate decides."""
    assert gen.compact_ok(TEMPLATE, 1) and len(TEMPLATE) == 24
    rng = random.Random(max_len)
    pair_ref = PairRef(oracle, TEMPLATE, 2, EDGE_POOL, 1)
    for n1, n2 in ((max_len, 60), (60, max_len)):
        kinds = edge_kinds(rng, TEMPLATE, EDGE_POOL, n1, n2, False, False)
        picks = [kinds[i % len(kinds)] for i in range(260)]
        check_batch(sc, pair_ref, TEMPLATE, 2, EDGE_POOL, 1, [p[0] for p in picks], [p[1] for p in picks], (True, True), (n1, n2))


# ---- modes of leaving the kernel -----------------------------------------------------------------------------------------
def plan_batch(n=600, seed=5):
    rng = random.Random(seed)
    kinds = edge_kinds(rng, TEMPLATE, EDGE_POOL, 70, 55, True, True)
    picks = [kinds[rng.randrange(len(kinds))] for _ in range(n)]
    return [p[0] for p in picks], [p[1] for p in picks]


def test_tally_and_atomics_agree(sc, oracle, gpu, engine, monkeypatch):
    reads1, reads2 = plan_batch()
    pair_ref = PairRef(oracle, TEMPLATE, 2, EDGE_POOL, 1)
    for use_first, mode in MODES:
        expect = pair_ref.counts(reads1, reads2, use_first)
        for tally in ("0", "1"):
            monkeypatch.setenv("SCG_TALLY", tally)
            counts, total = run_plan(sc, TEMPLATE, 2, EDGE_POOL, 1, use_first, reads1, reads2)
            assert total == len(reads1) and np.array_equal(counts, expect), (mode, tally)


def test_batches_accumulate_reset_and_bind(sc, oracle, gpu, engine):
    import torch
    reads1, reads2 = plan_batch(400, 6)
    more1, more2 = plan_batch(300, 7)
    pair_ref = PairRef(oracle, TEMPLATE, 2, EDGE_POOL, 1)
    first, second = pair_ref.counts(reads1, reads2, False), pair_ref.counts(more1, more2, False)
    with sc.Plan.single_paired(TEMPLATE, 2, EDGE_POOL, 1, False, device=0) as plan:
        count_plan(sc, plan, reads1, reads2)
        count_plan(sc, plan, more1, more2)
        counts, total = plan.read()
        assert total == 700 and np.array_equal(counts[:len(EDGE_POOL)], first + second)
        plan.reset()
        counts, total = plan.read()
        assert total == 0 and not counts.any()
        count_plan(sc, plan, more1, more2)
        counts, total = plan.read()
        assert total == 300 and np.array_equal(counts[:len(EDGE_POOL)], second)
        mine = torch.zeros(len(EDGE_POOL), dtype=torch.int32, device="cuda:0")
        plan.bind_counters(mine)
        count_plan(sc, plan, reads1, reads2)
        plan.read()
        assert np.array_equal(mine.cpu().numpy(), first)
        plan.bind_counters(None)
        counts, _ = plan.read()
        assert np.array_equal(counts[:len(EDGE_POOL)], second)


# ---- files ---------------------------------------------------------------------------------------------------------------
def file_case():
    rng = random.Random(31)
    pool = gen.make_pool(rng, 40, 8, "ACGT", min_dist=2)
    reads1 = gen.make_reads(rng, TEMPLATE, [pool], 1400, 2, 0.03, 0.01, 0.02, 0.2, 40)
    return pool, reads1, ref.make_mates(rng, reads1)


_file_expect = {}


def file_expect(oracle):
    if not _file_expect:
        pool, reads1, reads2 = file_case()
        for use_first, mode in MODES:
            _file_expect[mode] = ref.count_single_paired(oracle, reads1, reads2, TEMPLATE, 2, pool, 1, use_first)
    return _file_expect


@pytest.mark.parametrize("window_kb", [None, 8])
def test_every_input_form(sc, oracle, gpu, engine, tmp_path, monkeypatch, window_kb):
    pool, reads1, reads2 = file_case()
    expect = file_expect(oracle)
    forms = {form: write_mates(tmp_path, reads1, reads2, form) for form in ("plain", "bgzf", "gzip")}
    if window_kb:
        monkeypatch.setenv("SCG_WINDOW_KB", str(window_kb))
    for first_form, second_form in (("plain", "plain"), ("bgzf", "bgzf"), ("gzip", "gzip"), ("plain", "bgzf"), ("gzip", "plain")):
        p1, p2 = forms[first_form][0], forms[second_form][1]
        for use_first, mode in MODES:
            counts, total = sc.count_single_barcodes_paired(p1, p2, TEMPLATE, 2, pool, 1, use_first, 4)
            assert total == expect[mode][1] == len(reads1), (first_form, second_form, mode)
            assert np.array_equal(counts, expect[mode][0]), (first_form, second_form, mode)
    # the host readers alone
    monkeypatch.setenv("SCG_DEVICE_SCAN", "0")
    counts, total = sc.count_single_barcodes_paired(forms["plain"][0], forms["gzip"][1], TEMPLATE, 2, pool, 1, False, 4)
    assert total == len(reads1) and np.array_equal(counts, expect["best"][0])


def test_unequal_read_counts(sc, gpu, engine, tmp_path):
    from screencounter_amd import _lib
    pool, reads1, reads2 = file_case()
    p1, p2 = write_mates(tmp_path, reads1, reads2[:-7])
    for a, b in ((p1, p2), (p2, p1)):
        with pytest.raises(sc.ScgError) as e:
            sc.count_single_barcodes_paired(a, b, TEMPLATE, 2, pool, 1, True, 4)
        assert e.value.code == _lib.SCG_ERR_IO and "different number of reads in paired FASTQ files" in str(e.value)


def test_two_pipelines_on_one_device(sc, oracle, gpu, engine, tmp_path, monkeypatch):
    pool, reads1, reads2 = file_case()
    expect = file_expect(oracle)
    p1, p2 = write_mates(tmp_path, reads1, reads2)
    monkeypatch.setenv("SCG_WINDOW_KB", "16")
    monkeypatch.setenv("SCG_DEVICES", "0,0")
    for use_first, mode in MODES:
        counts, total = sc.count_single_barcodes_paired(p1, p2, TEMPLATE, 2, pool, 1, use_first, 4)
        assert total == len(reads1) and np.array_equal(counts, expect[mode][0]), mode


def test_many_files_give_what_one_file_gives(sc, gpu, engine, tmp_path):
    from screencounter_amd import _lib
    pool, reads1, reads2 = file_case()
    cuts = [(0, 500), (500, 501), (501, 501), (501, 1400)]              # (one pair; no pair at all)
    forms = ["plain", "bgzf", "gzip", "plain"]
    files = [write_mates(tmp_path, reads1[a:b], reads2[a:b], form, stem=f"f{k}_") for k, ((a, b), form) in enumerate(zip(cuts, forms))]
    paths1, paths2 = [f[0] for f in files], [f[1] for f in files]
    for use_first, mode in MODES:
        for devices in (None, [0, 0]):
            counts, totals = sc.count_single_barcodes_paired_files(paths1, paths2, TEMPLATE, 2, pool, 1, use_first, 4, devices=devices)
            assert counts.shape == (len(pool), len(files)) and totals == [b - a for a, b in cuts]
            for k, (p1, p2) in enumerate(files):
                one, total = sc.count_single_barcodes_paired(p1, p2, TEMPLATE, 2, pool, 1, use_first, 4)
                assert total == totals[k] and np.array_equal(counts[:, k], one), (mode, devices, k)
    # the lowest-numbered failing file is the one reported
    short = write_mates(tmp_path, reads1[:50], reads2[:40], stem="short_")
    gone = str(tmp_path / "gone.fastq")
    with pytest.raises(sc.ScgError) as e:
        sc.count_single_barcodes_paired_files([paths1[0], short[0], gone], [paths2[0], short[1], gone], TEMPLATE, 2, pool, 1, True, 4)
    assert e.value.code == _lib.SCG_ERR_IO and "different number of reads in paired FASTQ files" in str(e.value)
    with pytest.raises(sc.ScgError) as e:
        sc.count_single_barcodes_paired_files([paths1[0], gone, short[0]], [paths2[0], paths2[1], short[1]], TEMPLATE, 2, pool, 1, True, 4)
    assert e.value.code == _lib.SCG_ERR_IO and "gone.fastq" in str(e.value)
