"""Combinations over any number of variable regions on the GPU: Plan.combo_regions on uploaded reads and the two file
entries, on the staged and the byte-wise engine (SCG_FORCE_GENERAL=1), with dense cells and with key streams
(SCG_DENSE_CELLS=0), compared exactly with what the real kaori::CombinatorialBarcodesSingleEnd<256, V> counted
(tests/golden/kaori_combo_regions.json) or with its restatement (tests/combo_regions_ref.py, pinned to those goldens by
test_combo_regions_reference_cpu.py).  Constructed inputs say what a wrong stride, slot, budget or tie rule would change;
the tile and dispatch edges are those of tests/test_gpu_tile_edges.py, for three-region templates that reach each of the
18 (NW, NT, NC, W) cells of combo_regions_staged_kernel and for one eight-region template."""
import itertools
import random

import numpy as np
import pytest

from oracle.pyoracle import write_fastq
from tests import combo_regions_ref as ref
from tests import gen
from tests import golden_util as G
from tests import test_gpu_tile_edges as TE

pytestmark = pytest.mark.gpu

CASES = G.load("kaori_combo_regions.json")
ACCEPTED = [c for c in CASES if "error" not in c["expect"]["best"]]
WORKGROUP = 256                         # reads per workgroup of the staged kernels (STAGE_BLOCK)


def engine(monkeypatch, general):
    if general:
        monkeypatch.setenv("SCG_FORCE_GENERAL", "1")
    else:
        monkeypatch.delenv("SCG_FORCE_GENERAL", raising=False)


def dense(monkeypatch, on):
    if on:
        monkeypatch.delenv("SCG_DENSE_CELLS", raising=False)
    else:
        monkeypatch.setenv("SCG_DENSE_CELLS", "0")


def count_plan(sc, gpu, reads, template, strand, pools, mismatches, use_first, hint=0, fixed_len=0):
    """(combinations as rows [i_0, ..., i_last, count], total) of one batch through Plan.combo_regions."""
    with sc.Plan.combo_regions(template, strand, pools, mismatches, use_first, device=0) as plan:
        if fixed_len:
            seqs, _ = sc.upload_reads(reads, gpu)
            plan.count(seqs, fixed_len=fixed_len, n_reads=len(reads))
        else:
            seqs, offs = sc.upload_reads(reads, gpu)
            plan.count(seqs, offs, max_len=hint)
        idx, freq, total = plan.read_combinations()
    assert idx.shape == (len(pools), len(freq)) and idx.dtype == np.int32
    return ref.indices_list(idx, freq), total


def count_file(sc, path, template, strand, pools, mismatches, use_first):
    idx, freq, total = sc.count_combo_barcodes_regions(str(path), template, strand, pools, mismatches, use_first)
    assert idx.shape == (len(pools), len(freq))
    return ref.indices_list(idx, freq), total


def expected(oracle, reads, template, strand, pools, mismatches, use_first):
    idx, freq, total = ref.count_combo_regions(oracle, reads, template, strand, pools, mismatches, use_first)
    return ref.indices_list(idx, freq), total


def group_of(case):
    """The golden's group: the name in front of its number ("V3[14]" -> "V3"; V1 .. V8, wide, big, ties, rejected)."""
    return G.case_id(case).split("[")[0]


GROUPS = sorted({group_of(c) for c in CASES})


# ---- 1. the goldens, through the plan and the file entry, both modes, both engines ------------------------------------------
# (one test per group of goldens and mode, every case of the group in it: a failure names the case)
@pytest.mark.parametrize("use_first", [True, False], ids=["first", "best"])
@pytest.mark.parametrize("group", GROUPS)
def test_goldens(sc, gpu, tmp_path, monkeypatch, group, use_first):
    cases = [c for c in CASES if group_of(c) == group]
    assert cases
    for case in cases:
        name = G.case_id(case)
        expect = case["expect"]["first" if use_first else "best"]
        args = (case["template"], case["strand"], case["pools"], case["mismatches"], use_first)
        path = tmp_path / "reads.fastq"
        write_fastq(str(path), case["reads"])
        for general in (False, True):
            engine(monkeypatch, general)
            if "error" in expect:
                for call in (lambda: count_plan(sc, gpu, case["reads"], *args), lambda: count_file(sc, path, *args)):
                    with pytest.raises(sc.ScgError) as e:
                        call()
                    assert str(e.value) == expect["error"], name
                continue
            want = (expect["combinations"], expect["total"])
            assert count_plan(sc, gpu, case["reads"], *args) == want, f"{name}: plan, general={general}"
            assert count_file(sc, path, *args) == want, f"{name}: file, general={general}"


# ---- 3. dense cells and key streams give one list ----------------------------------------------------------------------------
@pytest.mark.parametrize("group", sorted({group_of(c) for c in ACCEPTED}))
def test_goldens_as_key_streams(sc, gpu, tmp_path, monkeypatch, group):
    dense(monkeypatch, False)
    cases = [c for c in ACCEPTED if group_of(c) == group]
    assert cases
    for case in cases:
        name = G.case_id(case)
        path = tmp_path / "reads.fastq"
        write_fastq(str(path), case["reads"])
        for use_first in (True, False):
            expect = case["expect"]["first" if use_first else "best"]
            args = (case["template"], case["strand"], case["pools"], case["mismatches"], use_first)
            for general in (False, True):
                engine(monkeypatch, general)
                with sc.Plan.combo_regions(*args, device=0) as plan:
                    assert plan.num_counters == 0, name
                assert count_plan(sc, gpu, case["reads"], *args) == (expect["combinations"], expect["total"]), f"{name}: plan, general={general}"
            assert count_file(sc, path, *args) == (expect["combinations"], expect["total"]), f"{name}: file"


def test_every_golden_is_in_a_group():
    assert sum(len([c for c in CASES if group_of(c) == g]) for g in GROUPS) == len(CASES) == 58
    assert sum(len([c for c in ACCEPTED if group_of(c) == g]) for g in GROUPS) == len(ACCEPTED) == 53


# ---- 2. two regions: the existing combination plan and entry ----------------------------------------------------------------
@pytest.mark.parametrize("seed", range(9))
def test_two_regions_equal_the_existing_handler(sc, gpu, tmp_path, monkeypatch, seed):
    rng = random.Random(5200 + seed)
    c = gen.random_combo_case(rng, sizes=(200, 700), wide={0: False, 1: True, 2: "big"}[seed % 3])
    pools = [c["pool0"], c["pool1"]]
    path = tmp_path / "reads.fastq"
    write_fastq(str(path), c["reads"])
    seqs, offs = sc.upload_reads(c["reads"], gpu)
    for on in (True, False):                                   # dense cells, then key streams
        dense(monkeypatch, on)
        for use_first in (True, False):
            try:
                with sc.Plan.combo(c["template"], c["strand"], c["pool0"], c["pool1"], c["mismatches"], use_first, device=0) as plan:
                    plan.count(seqs, offs)
                    idx, freq, total = plan.read_combo()
            except sc.ScgError as rejected:                    # (random IUPAC codes that expand to one sequence twice)
                with pytest.raises(sc.ScgError) as e:
                    count_plan(sc, gpu, c["reads"], c["template"], c["strand"], pools, c["mismatches"], use_first)
                assert str(e.value) == str(rejected)
                continue
            want = (ref.indices_list(idx, freq), total)
            assert total == len(c["reads"])
            assert count_plan(sc, gpu, c["reads"], c["template"], c["strand"], pools, c["mismatches"], use_first) == want, (on, use_first)
            old = sc.count_combo_barcodes_single(str(path), c["template"], c["strand"], pools, c["mismatches"], use_first)
            assert (ref.indices_list(old[0], old[1]), old[2]) == want, (on, use_first)
            assert count_file(sc, path, c["template"], c["strand"], pools, c["mismatches"], use_first) == want, (on, use_first)


# ---- 4. keys beyond 32 bits ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("general", [False, True], ids=["staged", "general"])
def test_keys_beyond_32_bits(sc, gpu, oracle, monkeypatch, general):
    """Three pools of 1 700 sequences: 4.9e9 combinations > 2^32, the first pool's stride 2.89e6 and the top key 4.9e9.  Reads
    sit on the highest index of every pool and on mixtures of highest and lowest: a stride or a key kept in 32 bits lands
    elsewhere."""
    engine(monkeypatch, general)
    rng = random.Random(64)
    every = ["".join(p) for p in itertools.product("ACGT", repeat=6)]
    pools = []
    for _ in range(3):
        rng.shuffle(every)
        pools.append(list(every[:1700]))
    template = "CAGT------TTAC------GGCA------ACTG"
    top = 1699
    planted = [(top, top, top)] * 5 + [(top, 0, top)] * 3 + [(0, top, 0)] * 2 + [(top, top, 0)] * 4 + [(1, 2, 3)] + [(top - 1, top, top - 2)] * 6
    fill = gen.Filler(640)
    reads = []
    for k, combo in enumerate(planted):
        construct = gen.fill_template(template, [pools[r][i] for r, i in enumerate(combo)])
        read = gen.place(fill, construct, 60, k % 20)
        reads.append(gen.rc(read) if k % 2 else read)
    reads += [fill(50) for _ in range(300)]
    rng.shuffle(reads)
    want = sorted([list(c) + [planted.count(c)] for c in set(planted)])
    for use_first in (True, False):
        got, total = count_plan(sc, gpu, reads, template, 2, pools, 0, use_first)
        assert got == want and total == len(reads)
        assert expected(oracle, reads, template, 2, pools, 0, use_first) == (want, len(reads))


# ---- 5. strand and slot order --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("on", [True, False], ids=["dense", "stream"])
@pytest.mark.parametrize("general", [False, True], ids=["staged", "general"])
def test_reverse_strand_meets_the_pools_back_to_front(sc, gpu, oracle, monkeypatch, general, on):
    """Pools of 2, 3 and 5 sequences of 5, 6 and 7 bases, reverse strand only: combination (a, b, c) is planted a * 15 + b * 5
    + c + 1 times, so that every cell has its own count; a pool looked up in the wrong slot finds nothing (the lengths
    differ) and a wrong stride moves counts between cells."""
    engine(monkeypatch, general)
    dense(monkeypatch, on)
    rng = random.Random(235)
    pools = [gen.make_pool(rng, n, v, gen.BASES, min_dist=3) for n, v in ((2, 5), (3, 6), (5, 7))]
    template = "ACGTAC-----GT------CATG-------TGCA"
    fill = gen.Filler(235)
    reads, want = [], []
    for a, b, c in itertools.product(range(2), range(3), range(5)):
        n = a * 15 + b * 5 + c + 1
        want.append([a, b, c, n])
        construct = gen.fill_template(template, [pools[0][a], pools[1][b], pools[2][c]])
        reads += [gen.rc(gen.place(fill, construct, 50 + k % 7, k % 5)) for k in range(n)]
    rng.shuffle(reads)
    for use_first in (True, False):
        assert count_plan(sc, gpu, reads, template, 1, pools, 1, use_first) == (want, len(reads))
        assert count_plan(sc, gpu, reads, template, 0, pools, 1, use_first) == ([], len(reads))      # (nothing on the forward strand)
    assert expected(oracle, reads, template, 1, pools, 1, False) == (want, len(reads))


# ---- 6. one budget for the constant bases and all regions ------------------------------------------------------------------
@pytest.mark.parametrize("general", [False, True], ids=["staged", "general"])
def test_the_budget_is_shared(sc, gpu, oracle, monkeypatch, general):
    engine(monkeypatch, general)
    rng = random.Random(66)
    pools = [gen.make_pool(rng, 6, 8, gen.BASES, min_dist=4) for _ in range(3)]
    template = "GATTACA--------CC--------TTGACG--------AGT"
    fill = gen.Filler(66)
    regs = ref.regions_of(template)
    construct = gen.fill_template(template, [pools[0][1], pools[1][2], pools[2][3]])
    two = gen.substitute(gen.substitute(construct, regs[0][0] + 2), regs[2][0] + 5)        # one substitution in each of two regions
    three = gen.substitute(two, 3)                                                         # ... and one in a constant base
    one_each = gen.substitute(gen.substitute(construct, regs[1][0]), 1)                    # a region and a constant base
    for strand_of_read in (lambda s: s, gen.rc):
        for use_first in (True, False):
            def counted(read, budget):
                reads = [strand_of_read(gen.place(fill, read, 70, 9)), fill(64)]
                got = count_plan(sc, gpu, reads, template, 2, pools, budget, use_first)
                assert got == expected(oracle, reads, template, 2, pools, budget, use_first)
                assert got[1] == 2 and got[0] in ([], [[1, 2, 3, 1]])
                return bool(got[0])
            assert counted(two, 2) and not counted(two, 1)
            assert not counted(three, 2) and counted(three, 3)
            assert counted(one_each, 2) and not counted(one_each, 1)


# ---- 7. the best-mode rule ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("on", [True, False], ids=["dense", "stream"])
@pytest.mark.parametrize("general", [False, True], ids=["staged", "general"])
def test_best_mode_ties_and_first_mode(sc, gpu, oracle, monkeypatch, general, on):
    engine(monkeypatch, general)
    dense(monkeypatch, on)
    rng = random.Random(77)
    pools = [gen.make_pool(rng, 5, 7, gen.BASES, min_dist=4) for _ in range(3)]
    template = "TCAGGA-------AC-------GTTC-------CAT"
    fill = gen.Filler(77)
    regs = ref.regions_of(template)

    def construct(a, b, c):
        return gen.fill_template(template, [pools[0][a], pools[1][b], pools[2][c]])

    def both(first, second):
        return fill(3) + first + fill(5) + second + fill(2)
    cases = {
        "equal totals, different combinations": (both(construct(0, 1, 2), construct(3, 1, 2)), [[0, 1, 2, 1]], []),
        "equal totals, the same combination": (both(construct(4, 0, 1), construct(4, 0, 1)), [[4, 0, 1, 1]], [[4, 0, 1, 1]]),
        "the later construct is closer": (both(gen.substitute(construct(2, 2, 2), regs[1][0] + 1), construct(1, 3, 4)), [[2, 2, 2, 1]], [[1, 3, 4, 1]]),
        "the earlier construct is closer": (both(construct(2, 0, 0), gen.substitute(construct(1, 3, 4), regs[2][0])), [[2, 0, 0, 1]], [[2, 0, 0, 1]]),
        "three constructs, the tie is between the worse two": (both(gen.substitute(construct(0, 0, 0), 0), construct(3, 3, 3)) +
                                                               gen.substitute(construct(1, 1, 1), 2), [[0, 0, 0, 1]], [[3, 3, 3, 1]]),
    }
    for name, (read, first, best) in cases.items():
        for r in (read, gen.rc(read)):
            if r != read:                                      # (the reverse complement meets the constructs in the other order)
                first = {"the later construct is closer": [[1, 3, 4, 1]], "the earlier construct is closer": [[1, 3, 4, 1]],
                         "equal totals, different combinations": [[3, 1, 2, 1]],
                         "three constructs, the tie is between the worse two": [[1, 1, 1, 1]]}.get(name, first)
            reads = [fill(40), r]
            assert count_plan(sc, gpu, reads, template, 2, pools, 1, True) == (first, 2), (name, "first")
            assert count_plan(sc, gpu, reads, template, 2, pools, 1, False) == (best, 2), (name, "best")
            for use_first in (True, False):
                assert expected(oracle, reads, template, 2, pools, 1, use_first) == ((first if use_first else best), 2), name


# ---- 8. tile and dispatch edges -----------------------------------------------------------------------------------------------
def three_regions(segments):
    """A two-region layout of tests/test_gpu_tile_edges.py with its last region cut in two around a 2-base spacer: the same
    length, the same constant runs at both ends, three regions."""
    k = max(i for i, (kind, _) in enumerate(segments) if kind == TE.V)
    n = segments[k][1]
    a = (n - 2) // 2
    return segments[:k] + [(TE.V, a), (TE.C, 2), (TE.V, n - 2 - a)] + segments[k + 1:]


def _cells():
    cells = []
    for w in (TE.U32, TE.U64):
        for nw, nt, nc in TE.SHAPES:
            segs, hint = TE.COMBO[(nw, nt, nc, w)]
            t = gen.segments_template(random.Random(f"regions{nw}{nt}{nc}{w}"), three_regions(segs))
            cells.append(dict(nw=nw, nt=nt, nc=nc, w=w, t=t, hint=hint, mm=TE._pick_mm(t, nw, nc, nt)))
    for (nw, nt, nc), (segs, hint) in TE.DSE8.items():
        t = gen.segments_template(random.Random(nt * 37 + nw), segs)
        cells.append(dict(nw=nw, nt=nt, nc=nc, w=TE.U32, t=t, hint=hint, mm=TE._pick_mm(t, nw, nc, nt)))
    for c in cells:
        c["id"] = f"V{len(ref.regions_of(c['t']))}-NW{c['nw']}-NT{c['nt']}-NC{c['nc']}-{'u32' if c['w'] == TE.U32 else 'u64'}-T{len(c['t'])}-h{c['hint']}"
    return cells


CELLS = _cells()


def host_kernel(cell):
    """The staged kernel the host launches for the cell (a mirror of launch_combo_regions and LaunchComboRegions)."""
    t, h = cell["t"], cell["hint"]
    nw = 5 if h <= 160 else 10
    nt = 2 if len(t) <= 64 else 4 if len(t) <= 128 else 8
    nc = 3 if nw == 5 and gen.compact_ok(t, cell["mm"]) and h - len(t) + 1 <= 96 else nw
    w = TE.U64 if any(b - a > 32 for a, b in ref.regions_of(t)) else TE.U32
    return f"combo_regions_staged_kernel<{nw}, {nt}, {nc}, {w}>"


def test_cell_table_reaches_every_cell():
    seen = set()
    for c in CELLS:
        assert host_kernel(c) == f"combo_regions_staged_kernel<{c['nw']}, {c['nt']}, {c['nc']}, {c['w']}>", c["id"]
        assert len(ref.regions_of(c["t"])) in (3, 8) and max(b - a for a, b in ref.regions_of(c["t"])) <= 64
        seen.add(host_kernel(c))
    assert len(seen) == 18 and sum(len(ref.regions_of(c["t"])) == 8 for c in CELLS) == 3


@pytest.mark.parametrize("cell", CELLS, ids=[c["id"] for c in CELLS])
def test_tile_and_dispatch_edges(sc, gpu, oracle, cell):
    t, H, mm = cell["t"], cell["hint"], cell["mm"]
    T = len(t)
    rng = random.Random(cell["id"])
    fill = gen.Filler(len(cell["id"]) * 131 + T)
    regs = ref.regions_of(t)
    pools = [gen.make_pool(rng, 3 + r % 3, b - a, gen.BASES, min_dist=min(3, max(1, (b - a) // 2))) for r, (a, b) in enumerate(regs)]
    serial = itertools.count()

    def construct():
        k = next(serial)
        return gen.fill_template(t, [p[(k + r) % len(p)] for r, p in enumerate(pools)])
    edge = []
    for f in (lambda s: s, gen.rc):
        edge += [gen.place(fill, f(construct()), H, 0), gen.place(fill, f(construct()), H, H - T),          # both ends of a read
                 f(construct()), f(construct())[:-1], f(construct())[1:], ""]                                # T, T - 1 and 0 bases
        lone = construct()
        edge.append(gen.place(fill, f(gen.substitute(lone, regs[-1][0] + 1, "N")), min(H, T + 9), min(H - T, 4)))   # a lone N in a region
        if mm:
            edge.append(gen.place(fill, f(gen.substitute(construct(), regs[0][0])), H, (H - T) // 2))
        if 2 * T + 1 <= H:
            edge.append(f(construct() + "A" + construct()))
    reads = list(edge)
    while len(reads) < WORKGROUP + 1:                          # one workgroup's reads + 1, constructs in a third of them
        n = rng.randint(0, H)
        reads.append(gen.place(fill, construct(), n, rng.randint(0, n - T)) if n >= T and rng.random() < 0.33 else fill(n))
    per_read = {uf: ref.read_combinations(oracle, reads, t, 2, pools, mm, uf) for uf in (True, False)}

    def want(n, uf, of=None):
        tally = {}
        for combo in (per_read[uf][:n] if of is None else of):
            if combo is not None:
                tally[combo] = tally.get(combo, 0) + 1
        return [list(k) + [tally[k]] for k in sorted(tally)], n
    assert want(len(edge), True)[0], "the constructed reads hold nothing to count"
    for uf in (True, False):
        for n in (WORKGROUP - 1, WORKGROUP, WORKGROUP + 1, len(edge)):                                       # ragged batches
            assert count_plan(sc, gpu, reads[:n], t, 2, pools, mm, uf, hint=H) == want(n, uf), (n, uf)
        fixed = [r for r in reads if len(r) == H]                                                             # a fixed-length batch
        fixed_want = want(len(fixed), uf, [c for r, c in zip(reads, per_read[uf]) if len(r) == H])
        assert len(fixed) >= 4 and count_plan(sc, gpu, fixed, t, 2, pools, mm, uf, fixed_len=H) == fixed_want, uf


# ---- 9. the plan's life -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("on", [True, False], ids=["dense", "stream"])
def test_plan_accumulates_and_resets(sc, gpu, oracle, monkeypatch, on):
    dense(monkeypatch, on)
    rng = random.Random(91)
    c = ref.make_case(rng, (5, 7, 6), (3, 4, 5), 600, 2, 1)
    args = (c["template"], c["strand"], c["pools"], c["mismatches"], False)
    a, b = c["reads"][:250], c["reads"][250:]
    with sc.Plan.combo_regions(*args, device=0) as plan:
        assert plan.num_counters == (60 if on else 0)
        for part in (a, b):
            plan.count(*sc.upload_reads(part, gpu))
        idx, freq, total = plan.read_combinations()
        assert (ref.indices_list(idx, freq), total) == expected(oracle, c["reads"], *args)
        assert plan.read()[1] == 600 and (not on or int(plan.read()[0].sum()) == int(freq.sum()))
        plan.reset()
        assert plan.read_combinations()[1].size == 0 and plan.read()[1] == 0
        plan.count(*sc.upload_reads(b, gpu))
        idx, freq, total = plan.read_combinations()
        assert (ref.indices_list(idx, freq), total) == expected(oracle, b, *args)


@pytest.mark.parametrize("on", [True, False], ids=["dense", "stream"])
def test_files_and_devices(sc, gpu, oracle, tmp_path, monkeypatch, on):
    """Two pipelines on one card (SCG_DEVICES=0,0) give what one gives; the many-files entry gives what the one-file entry
    gives for each file, the plan being reset in between; plain, BGZF and gzip inputs give the same."""
    dense(monkeypatch, on)
    rng = random.Random(92)
    c = ref.make_case(rng, (6, 4, 8, 5), (4, 2, 3, 5), 1500, 2, 2)
    args = (c["template"], c["strand"], c["pools"], c["mismatches"], False)
    parts = [c["reads"][:700], c["reads"][700:1097], c["reads"][1097:1100], c["reads"][1100:]]
    paths = []
    for k, part in enumerate(parts):
        text = gen.fastq_text(part)
        path = tmp_path / f"part{k}.{('fastq', 'fastq.gz', 'fastq', 'fastq.gz')[k]}"
        if k == 1:
            gen.write_bgzf(str(path), text, block=3000)
        elif k == 3:
            write_fastq(str(path), part, gz=True)
        else:
            path.write_bytes(text)
        paths.append(str(path))
    want = [expected(oracle, part, *args) for part in parts]
    one = [count_file(sc, p, *args) for p in paths]
    assert one == want
    plain = tmp_path / "part1.fastq"
    plain.write_bytes(gen.fastq_text(parts[1]))
    assert count_file(sc, plain, *args) == want[1]
    many = sc.count_combo_barcodes_regions_files(paths, *args)
    assert [(ref.indices_list(i, f), t) for i, f, t in many] == want
    monkeypatch.setenv("SCG_DEVICES", "0,0")
    assert [count_file(sc, p, *args) for p in paths] == want
    many = sc.count_combo_barcodes_regions_files(paths, *args)
    assert [(ref.indices_list(i, f), t) for i, f, t in many] == want
