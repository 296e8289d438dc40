"""scg_count_combo_barcodes_single_matrix and scg_count_combo_barcodes_paired_matrix: matrixOfComboBarcodes and
matrixOfPairedComboBarcodes in one native call, the files' combinations merged on the device.  The matrix must be
combineComboCounts -- the numpy restatement of tests/combo_matrix_ref.py -- of the per-file results of the existing *_files
entry, and of the oracle's per-file results, whatever the storage of the grid (dense cells compacted on the device, or the
sorted runs of sparse mode), the devices, the kernels (staged or general), the mode and the strand.

A plate is four small files: plain, gzip, BGZF; one has no match, the last one repeats the first."""
import gzip
import random

import numpy as np
import pytest

from tests import combo_matrix_ref as ref
from tests import gen

pytestmark = pytest.mark.gpu

T = ref.tile_cells()
T_COMBO = "AGCTTA" + "-" * 8 + "GGTACA" + "-" * 9 + "CCATGA"
T_MATE1 = "CAGT" + "-" * 10 + "GGA"
T_MATE2 = "TTAC" + "-" * 9 + "CCT"
PLATE = [("mixed", 400, "plain"), ("none", 300, "gzip"), ("mixed", 350, "bgzf"), ("copy of 0", 400, "gzip")]
NONE, COPY = 1, 3


def pad(rng, construct, rev=False):
    read = gen.rand_seq(rng, rng.randint(0, 10)) + construct + gen.rand_seq(rng, rng.randint(0, 10))
    return gen.rc(read) if rev else read


def junk(rng):
    return gen.rand_seq(rng, rng.randint(2, 40))


def single_plate(seed=606):
    """Reads of T_COMBO on either strand over 25 x 23 barcodes, a few of them mutated."""
    rng = random.Random(seed)
    p0 = gen.make_pool(rng, 25, 8, "ACGT", min_dist=3)
    p1 = gen.make_pool(rng, 23, 9, "ACGT", min_dist=3)
    files = []
    for kind, n, _form in PLATE:
        if kind == "copy of 0":
            files.append(list(files[0]))
            continue
        reads = []
        for _ in range(n):
            if kind == "none" or rng.random() < 0.1:
                reads.append(junk(rng))
                continue
            core = gen.mutate(rng, gen.fill_template(T_COMBO, [rng.choice(p0[:12]), rng.choice(p1)]), 0.01, 0.003, 0.02)
            reads.append(pad(rng, core, rev=rng.random() < 0.5))
        files.append(reads)
    return dict(pools=[p0, p1], files=files)


def paired_plate(seed=707):
    """Mates of T_MATE1 / T_MATE2 (mate 2 on the reverse strand) over 20 x 18 barcodes; pool 2 has IUPAC codes."""
    rng = random.Random(seed)
    u1 = gen.make_pool(rng, 20, 10, "ACGT", min_dist=3)
    u2 = gen.make_pool(rng, 18, 9, "ACGT", min_dist=4, iupac_rate=0.12)
    files = []
    for kind, n, _form in PLATE:
        if kind == "copy of 0":
            files.append((list(files[0][0]), list(files[0][1])))
            continue
        r1, r2 = [], []
        for _ in range(n):
            u = 1.0 if kind == "none" else rng.random()
            a = gen.fill_template(T_MATE1, [rng.choice(u1)]) if u < 0.85 else None
            b = gen.fill_template(T_MATE2, [gen.concrete(rng, rng.choice(u2))]) if u < 0.75 or 0.85 <= u < 0.93 else None
            r1.append(pad(rng, gen.mutate(rng, a, 0.01, 0.003, 0.02)) if a else junk(rng))
            r2.append(pad(rng, gen.mutate(rng, b, 0.01, 0.003, 0.02), rev=True) if b else junk(rng))
        files.append((r1, r2))
    return dict(u1=u1, u2=u2, files=files)


SINGLE, PAIRED = single_plate(), paired_plate()


def write_form(path, reads, form):
    text = gen.fastq_text(reads)
    if form == "plain":
        path += ".fastq"
        open(path, "wb").write(text)
    elif form == "bgzf":
        path += ".fastq.gz"
        gen.write_bgzf(path, text, block=3000)
    else:
        path += ".fq.gz"
        with gzip.open(path, "wb") as f:
            f.write(text)
    return path


@pytest.fixture(scope="module")
def plates(tmp_path_factory):
    root = tmp_path_factory.mktemp("combo_matrix")
    single = [write_form(str(root / f"s_{f}"), SINGLE["files"][f], form) for f, (_k, _n, form) in enumerate(PLATE)]
    paired = [(write_form(str(root / f"m1_{f}"), PAIRED["files"][f][0], form), write_form(str(root / f"m2_{f}"), PAIRED["files"][f][1], form))
              for f, (_k, _n, form) in enumerate(PLATE)]
    return dict(single=single, paired=paired, root=root)


_oracle_cache = {}


def oracle_single(oracle, strand, use_first):
    """Per file (indices, freq, total) by the oracle: computed once per setting and left unchanged."""
    key = ("single", strand, use_first)
    if key not in _oracle_cache:
        _oracle_cache[key] = [oracle.count_combo(reads, T_COMBO, strand, *SINGLE["pools"], 1, use_first) for reads in SINGLE["files"]]
    return _oracle_cache[key]


def oracle_paired(oracle, use_first):
    key = ("paired", use_first)
    if key not in _oracle_cache:
        _oracle_cache[key] = [oracle.count_combo_paired(r1, r2, T_MATE1, False, 1, PAIRED["u1"], T_MATE2, True, 1, PAIRED["u2"], False, use_first)
                              for r1, r2 in PAIRED["files"]]
    return _oracle_cache[key]


@pytest.fixture(params=["dense", "sparse"])
def storage(request, monkeypatch):
    """The grid as cells (compacted on the device), or -- the dense limit at 0 cells -- as the sorted runs of sparse mode."""
    if request.param == "sparse":
        monkeypatch.setenv("SCG_DENSE_CELLS", "0")
    else:
        monkeypatch.delenv("SCG_DENSE_CELLS", raising=False)
    return request.param


@pytest.fixture(params=["staged", "general"])
def kernels(request, monkeypatch):
    if request.param == "general":
        monkeypatch.setenv("SCG_FORCE_GENERAL", "1")
    else:
        monkeypatch.delenv("SCG_FORCE_GENERAL", raising=False)
    return request.param


DEVICES = [None, [0], [0, 0, 0]]
MODES = [(True, 2), (False, 2), (True, 0), (False, 1)]      # (use_first, strand)


def test_the_plates_are_not_degenerate(oracle):
    per = oracle_single(oracle, 2, True)
    assert len(per[NONE][1]) == 0 and per[NONE][2] == PLATE[NONE][1]
    assert len(per[0][1]) > 100 and len(per[2][1]) > 100
    union, matrix = ref.combine([(i, f) for i, f, _t in per])
    assert matrix.shape[0] > max(len(per[0][1]), len(per[2][1]))          # the files differ
    assert np.array_equal(matrix[:, 0], matrix[:, COPY]) and not matrix[:, NONE].any()
    assert oracle_single(oracle, 0, True)[0][1].sum() < per[0][1].sum()   # reads on both strands
    pp = oracle_paired(oracle, True)
    assert len(pp[NONE]["freq"]) == 0 and len(pp[0]["freq"]) > 100 and pp[0]["barcode1_only"] > 0 and pp[0]["barcode2_only"] > 0
    assert any(set(b) - set("ACGT") for b in PAIRED["u2"])                # an IUPAC pool


@pytest.mark.parametrize("use_first,strand", MODES, ids=["first-both", "best-both", "first-forward", "best-reverse"])
@pytest.mark.parametrize("devices", DEVICES, ids=["default", "one", "three pipelines"])
def test_single_matrix(sc, gpu, oracle, plates, storage, kernels, devices, use_first, strand):
    args = (plates["single"], T_COMBO, strand, SINGLE["pools"], 1, use_first, 1, devices)
    indices, matrix, totals = sc.count_combo_barcodes_single_matrix(*args)
    per_file = sc.count_combo_barcodes_single_files(*args)
    ref.assert_matrix((indices, matrix), ref.combine([(i, f) for i, f, _t in per_file]))
    assert totals.tolist() == [t for _i, _f, t in per_file]
    expected = oracle_single(oracle, strand, use_first)
    ref.assert_matrix((indices, matrix), ref.combine([(i, f) for i, f, _t in expected]))
    assert totals.tolist() == [t for _i, _f, t in expected] == [n for _k, n, _form in PLATE]
    assert matrix.shape[1] == len(PLATE)


@pytest.mark.parametrize("use_first", [True, False], ids=["first", "best"])
@pytest.mark.parametrize("devices", DEVICES, ids=["default", "one", "three pipelines"])
def test_paired_matrix(sc, gpu, oracle, plates, storage, kernels, devices, use_first):
    p1, p2 = [a for a, _ in plates["paired"]], [b for _, b in plates["paired"]]
    args = (p1, T_MATE1, False, 1, PAIRED["u1"], p2, T_MATE2, True, 1, PAIRED["u2"], False, use_first, 1, devices)
    indices, matrix, totals, b1, b2 = sc.count_combo_barcodes_paired_matrix(*args)
    per_file = sc.count_combo_barcodes_paired_files(*args)
    ref.assert_matrix((indices, matrix), ref.combine([(i, f) for i, f, *_ in per_file]))
    assert [totals.tolist(), b1.tolist(), b2.tolist()] == [[r[k] for r in per_file] for k in (2, 3, 4)]
    expected = oracle_paired(oracle, use_first)
    ref.assert_matrix((indices, matrix), ref.combine([(d["indices"], d["freq"]) for d in expected]))
    assert [totals.tolist(), b1.tolist(), b2.tolist()] == [[d[k] for d in expected] for k in ("total", "barcode1_only", "barcode2_only")]


# ---- grids of T - 1, T and T + 1 cells, reads that hit the first and the last cell ------------------------------------
def near_square(total):
    d = max(d for d in range(1, int(total**0.5) + 1) if total % d == 0)
    return total // d, d


def distinct_barcodes(rng, n, length=8):
    return ["".join("ACGT"[(v >> (2 * i)) & 3] for i in range(length)) for v in rng.sample(range(4**length), n)]


@pytest.mark.parametrize("cells", [T - 1, T, T + 1], ids=["T-1", "T", "T+1"])
def test_grids_at_the_tile_edges(sc, gpu, oracle, tmp_path, cells):
    rng = random.Random(cells)
    n0, n1 = near_square(cells)
    p0, p1 = distinct_barcodes(rng, n0), distinct_barcodes(rng, n1, 9)
    hits = [(0, 0), (n0 - 1, n1 - 1), (0, n1 - 1), (n0 - 1, 0)] + [(rng.randrange(n0), rng.randrange(n1)) for _ in range(40)]
    files = [[pad(rng, gen.fill_template(T_COMBO, [p0[i], p1[j]])) for i, j in picks] for picks in (hits, hits[:2] * 3, hits[1:2])]
    paths = [write_form(str(tmp_path / f"edge_{f}"), reads, "plain") for f, reads in enumerate(files)]
    args = (paths, T_COMBO, 0, [p0, p1], 0, True, 1)
    indices, matrix, totals = sc.count_combo_barcodes_single_matrix(*args)
    expected = [oracle.count_combo(reads, T_COMBO, 0, p0, p1, 0, True) for reads in files]
    ref.assert_matrix((indices, matrix), ref.combine([(i, f) for i, f, _t in expected]))
    ref.assert_matrix((indices, matrix), ref.combine([(i, f) for i, f, _t in sc.count_combo_barcodes_single_files(*args)]))
    assert indices[:, 0].tolist() == [0, 0] and indices[:, -1].tolist() == [n0 - 1, n1 - 1]
    assert matrix[0].tolist() == [1, 3, 0] and matrix[-1].tolist() == [1, 3, 1] and totals.tolist() == [len(r) for r in files]


# ---- errors: the lowest-numbered failing file's message, and nothing handed out ---------------------------------------
def outcome(sc, fn, *args):
    with pytest.raises(sc.ScgError) as e:
        fn(*args)
    return e.value.code, str(e.value)


def test_single_matrix_errors(sc, gpu, plates, storage):
    good = plates["single"]
    missing = str(plates["root"] / "not_there.fastq")
    malformed = gen.write_flawed_fastq(str(plates["root"] / "malformed.fastq"), SINGLE["files"][2], {200: "malformed"})
    one = lambda path: outcome(sc, sc.count_combo_barcodes_single, path, T_COMBO, 2, SINGLE["pools"], 1, True, 1)
    many = lambda paths, devices=None: outcome(sc, sc.count_combo_barcodes_single_matrix, paths, T_COMBO, 2, SINGLE["pools"], 1, True, 1, devices)
    assert one(missing)[0] == sc._lib.SCG_ERR_IO and one(malformed)[0] == sc._lib.SCG_ERR_IO and one(missing) != one(malformed)
    for devices in DEVICES:
        assert many([good[0], missing, good[2], good[3]], devices) == one(missing)
        assert many([good[0], good[1], malformed, good[3]], devices) == one(malformed)
        assert many([good[0], good[1], malformed, missing], devices) == one(malformed)      # the lower-numbered one
        assert many([good[0], missing, malformed, good[3]], devices) == one(missing)
    # and the raw entry leaves nothing to free
    import ctypes as C
    from screencounter_amd import _lib
    junk_ = (C.c_int32 * 2)()
    idx, rows, freq, col, k = C.cast(junk_, _lib.i32_p), C.cast(junk_, _lib.i32_p), C.cast(junk_, _lib.i32_p), C.cast(junk_, _lib.i64_p), C.c_int64(9)
    farr = _lib.cstr_array([good[0], good[1], malformed, good[3]])[0]
    err = _lib.errbuf()
    rc = sc.load().scg_count_combo_barcodes_single_matrix(farr, 4, T_COMBO.encode(), 2, *_lib.pool(SINGLE["pools"][0]), *_lib.pool(SINGLE["pools"][1]),
                                                          1, 1, 1, C.byref(idx), C.byref(k), C.byref(col), C.byref(rows), C.byref(freq),
                                                          (C.c_int32 * 4)(), err, _lib.ERRCAP)
    assert rc == _lib.SCG_ERR_IO and not idx and not rows and not freq and not col and k.value == 0


def test_paired_matrix_errors(sc, gpu, plates, storage):
    good = plates["paired"]
    missing = str(plates["root"] / "not_there.fastq")
    short = write_form(str(plates["root"] / "short_mate"), PAIRED["files"][2][1][:-7], "plain")       # unequal mates
    malformed = gen.write_flawed_fastq(str(plates["root"] / "malformed_mate.fastq"), PAIRED["files"][2][1], {100: "malformed"})
    tail = (False, True, 1)

    def one(a, b):
        return outcome(sc, sc.count_combo_barcodes_paired, a, T_MATE1, False, 1, PAIRED["u1"], b, T_MATE2, True, 1, PAIRED["u2"], *tail)

    def many(pairs, devices=None):
        return outcome(sc, sc.count_combo_barcodes_paired_matrix, [a for a, _ in pairs], T_MATE1, False, 1, PAIRED["u1"],
                       [b for _, b in pairs], T_MATE2, True, 1, PAIRED["u2"], *tail, devices)

    unequal = one(good[2][0], short)
    assert "different number of reads" in unequal[1]
    for devices in DEVICES:
        assert many([good[0], (good[1][0], missing), good[2], good[3]], devices) == one(good[1][0], missing)
        assert many([good[0], good[1], (good[2][0], malformed), good[3]], devices) == one(good[2][0], malformed)
        assert many([good[0], good[1], (good[2][0], short), (missing, good[3][1])], devices) == unequal
