"""scg_count_random_barcodes_files: the files of matrixOfRandomBarcodes in one native call, every device keeping one tally in
HBM for all the files it takes (files mode: row ids, per-file harvest, soft reset, merge across devices).

The expectation is always the oracle's countRandomBarcodes applied to each file's reads, the union and the matrix built
as R/countRandomBarcodes.R:87-92 builds them; keys, matrix and totals must be equal, not close."""
import gzip
import os
import random

import numpy as np
import pytest

from tests import gen

pytestmark = pytest.mark.gpu

T_UNEQUAL = "GATCCA" + "-" * 10 + "TTG"            # flanks of 6 and 3: on the reverse strand the region sits at the FORWARD offset
T_EQUAL = "GATCCA" + "-" * 10 + "TTGCAG"


def expected(oracle, read_sets, template, strand, mismatches, use_first):
    tallies = [oracle.count_random(r, template, strand, mismatches, use_first) for r in read_sets]
    keys = sorted(set().union(*[t[0] for t in tallies])) if tallies else []
    row = {k: i for i, k in enumerate(keys)}
    matrix = np.zeros((len(keys), len(tallies)), dtype=np.int32)
    for c, (tally, _total) in enumerate(tallies):
        for k, v in tally.items():
            matrix[row[k], c] = v
    return keys, matrix, [t[1] for t in tallies]


def check(got, exp, what=""):
    keys, matrix, totals = got
    assert totals.tolist() == exp[2], what
    assert keys == exp[0], (what, len(keys), len(exp[0]), sorted(set(keys) ^ set(exp[0]))[:5])
    assert matrix.dtype == np.int32 and matrix.shape == exp[1].shape, what
    assert np.array_equal(matrix, exp[1]), (what, int(np.abs(matrix.astype(np.int64) - exp[1]).sum()))


def construct(rng, template, key, rev=False, pad=10, p_sub=0.0):
    core = gen.fill_template(template, [key])
    if p_sub:
        core = gen.mutate(rng, core, p_sub, 0.0, 0.0)
    read = gen.rand_seq(rng, rng.randint(0, pad)) + core + gen.rand_seq(rng, rng.randint(0, pad))
    return gen.rc(read) if rev else read


def reads_of(rng, template, keys, n, p_rev=0.5, p_junk=0.05, p_sub=0.0):
    out = []
    for _ in range(n):
        if rng.random() < p_junk:
            out.append(gen.rand_seq(rng, rng.randint(0, 50)))
        else:
            out.append(construct(rng, template, rng.choice(keys), rng.random() < p_rev, p_sub=p_sub))
    return out


def write_plain(path, reads):
    with open(path, "wb") as f:
        f.write(gen.fastq_text(reads))
    return str(path)


def write_as(path, reads, form):
    text = gen.fastq_text(reads)
    if form == "plain":
        with open(path, "wb") as f:
            f.write(text)
    elif form == "gzip":
        with gzip.open(path, "wb") as f:
            f.write(text)
    else:
        gen.write_bgzf(path, text, block=5000)
    return str(path)


# ---- overlap and empties ---------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def plate(tmp_path_factory):
    """Four files sharing about 40 keys: one without records, one in which no read matches, and one key that only the last
    file holds."""
    rng = random.Random(11)
    d = tmp_path_factory.mktemp("plate")
    keys = [gen.rand_seq(rng, 10) for _ in range(40)]
    only_last = "ACGTTGCAAC"
    assert only_last not in keys
    sets = [reads_of(rng, T_UNEQUAL, keys, 2000, p_sub=0.01),
            [],
            [gen.rand_seq(rng, rng.randint(0, 60), "AT") for _ in range(300)],      # (the template's C and G never occur)
            reads_of(rng, T_UNEQUAL, keys[:25], 700, p_sub=0.01) + [construct(rng, T_UNEQUAL, only_last, rev) for rev in (False, True, False)]]
    paths = [write_plain(d / f"s{i}.fastq", r) for i, r in enumerate(sets)]
    return paths, sets, only_last


@pytest.mark.parametrize("mismatches", [0, 1])
@pytest.mark.parametrize("use_first", [True, False])
@pytest.mark.parametrize("strand", [0, 1, 2])
def test_overlap_and_empties(sc, oracle, gpu, plate, strand, use_first, mismatches):
    paths, sets, only_last = plate
    exp = expected(oracle, sets, T_UNEQUAL, strand, mismatches, use_first)
    got = sc.count_random_barcodes_files(paths, T_UNEQUAL, strand, mismatches, use_first, 1)
    check(got, exp)
    keys, matrix, totals = got
    assert totals.tolist() == [2000, 0, 300, 703]
    assert not matrix[:, 1].any() and not matrix[:, 2].any()
    assert (matrix.sum(axis=1) > 0).all()                     # a key is a row only if some file counted it
    if strand != 1:
        i = keys.index(only_last)
        assert matrix[i, :3].tolist() == [0, 0, 0] and matrix[i, 3] > 0


def test_agrees_with_the_one_file_entry(sc, gpu, plate):
    paths, _sets, _only_last = plate
    keys, matrix, totals = sc.count_random_barcodes_files(paths, T_UNEQUAL, 2, 1, True, 1)
    for c, p in enumerate(paths):
        (seqs, freq), total = sc.count_random_barcodes(p, T_UNEQUAL, 2, 1, True, 1)
        column = {keys[i]: int(matrix[i, c]) for i in np.nonzero(matrix[:, c])[0]}
        assert column == dict(zip(seqs, freq.tolist())) and totals[c] == total, c


def test_one_file_in_a_list(sc, oracle, gpu, plate):
    paths, sets, _only_last = plate
    check(sc.count_random_barcodes_files(paths[:1], T_UNEQUAL, 2, 0, True, 1), expected(oracle, sets[:1], T_UNEQUAL, 2, 0, True))


# ---- key forms: packed up to 31 bases, hashed from 32; N and lower case hashed at any length ---------------------------
@pytest.mark.parametrize("form", ["plain", "gzip", "bgzf"])
@pytest.mark.parametrize("vlen", [8, 31, 32, 40])
def test_key_forms(sc, oracle, gpu, tmp_path, vlen, form):
    rng = random.Random(100 + vlen)
    template = "GATCCA" + "-" * vlen + "TTGCAG"
    keys = [gen.rand_seq(rng, vlen) for _ in range(30)]
    keys += [gen.rand_seq(rng, vlen, "ACGTN") for _ in range(5)] + [gen.rand_seq(rng, vlen, "ACGTacgtn") for _ in range(5)]
    sets = [reads_of(rng, template, keys, 600), reads_of(rng, template, keys[10:], 400), reads_of(rng, template, keys[:20] + keys[30:], 500)]
    paths = [write_as(tmp_path / f"k{i}.fastq{'' if form == 'plain' else '.gz'}", r, form) for i, r in enumerate(sets)]
    check(sc.count_random_barcodes_files(paths, template, 2, 0, True, 1), expected(oracle, sets, template, 2, 0, True))


# ---- growth between and inside files ---------------------------------------------------------------------------------
def test_rows_survive_growth(sc, oracle, gpu, tmp_path, monkeypatch):
    """One device, one table that starts at 2^16 slots.  File A's 40 000 keys push it past half; B re-counts 500 of them
    beside 500 new ones; C brings 70 000 more.  Small windows cut every file into several batches, so the table also
    grows in the middle of a file.  Ids given before a rehash must name the same keys after it."""
    monkeypatch.setenv("SCG_WINDOW_KB", "512")
    rng = random.Random(21)
    template = "ACGTAC" + "-" * 12 + "GTCA"
    distinct = set()
    while len(distinct) < 40000 + 500 + 70000:
        distinct.add(gen.rand_seq(rng, 12))
    distinct = sorted(distinct)
    rng.shuffle(distinct)
    a, new_b, c = distinct[:40000], distinct[40000:40500], distinct[40500:]
    b = rng.sample(a, 500) + new_b
    sets = [[construct(rng, template, k, pad=9) for k in ks] for ks in (a, b + b[:100], c)]
    paths = [write_plain(tmp_path / f"g{i}.fastq", r) for i, r in enumerate(sets)]
    exp = expected(oracle, sets, template, 0, 0, True)
    assert len(exp[0]) > 100000
    check(sc.count_random_barcodes_files(paths, template, 0, 0, True, 1, devices=[0]), exp)


# ---- more files than devices -------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def five(tmp_path_factory):
    rng = random.Random(31)
    d = tmp_path_factory.mktemp("five")
    keys = [gen.rand_seq(rng, 10, "ACGTn") for _ in range(60)]
    sets = [reads_of(rng, T_EQUAL, rng.sample(keys, 35), 300 + 350 * i) for i in range(5)]
    return [write_plain(d / f"f{i}.fastq", r) for i, r in enumerate(sets)], sets


def test_five_files_on_one_device(sc, oracle, gpu, five, monkeypatch):
    paths, sets = five
    monkeypatch.setenv("SCG_DEVICES", "0")
    check(sc.count_random_barcodes_files(paths, T_EQUAL, 2, 0, True, 1), expected(oracle, sets, T_EQUAL, 2, 0, True))


def test_five_files_on_two_tables_of_one_device(sc, oracle, gpu, five):
    """One card listed twice: two plans, each with its own table and ids, merged at the end like two devices."""
    paths, sets = five
    check(sc.count_random_barcodes_files(paths, T_EQUAL, 2, 0, True, 1, devices=[0, 0]), expected(oracle, sets, T_EQUAL, 2, 0, True))


def test_five_files_on_two_devices(sc, oracle, gpu, five):
    if sc.load().scg_device_count() < 2:
        pytest.skip("one device")
    paths, sets = five
    check(sc.count_random_barcodes_files(paths, T_EQUAL, 2, 0, True, 1, devices=[0, 1]), expected(oracle, sets, T_EQUAL, 2, 0, True))


# ---- forced collisions -----------------------------------------------------------------------------------------------
def hashed_plate(tmp_path, n_keys, seed):
    rng = random.Random(seed)
    template = "ACGTAC" + "-" * 12 + "TTGCAG"
    hashed = sorted({gen.rand_seq(rng, 12, "acgtN") for _ in range(n_keys * 3)})[:n_keys]
    packed = [gen.rand_seq(rng, 12) for _ in range(3)]
    sets = [reads_of(rng, template, hashed + packed, n, p_rev=0.0) for n in (900, 500, 700)]
    return template, [write_plain(tmp_path / f"h{i}.fastq", r) for i, r in enumerate(sets)], sets


def test_collisions_resolved(sc, oracle, gpu, tmp_path, monkeypatch):
    """Three hash bits: 8 tags per round for 12 hashed keys, so most of them collide in round 0 and are settled by the
    rounds behind it -- in the first file, and again (round 0 meets the slot of another key) in every later one."""
    template, paths, sets = hashed_plate(tmp_path, 12, 51)
    monkeypatch.setenv("SCG_TEST_RANDOM_TAG_BITS", "3")
    check(sc.count_random_barcodes_files(paths, template, 0, 0, True, 1, devices=[0]), expected(oracle, sets, template, 0, 0, True))


def test_collisions_exhausted(sc, gpu, tmp_path, monkeypatch):
    """No hash bits: a round settles one hashed key, four rounds cannot settle six.  The call fails with the plan
    read-out's error and hands nothing out."""
    from screencounter_amd import _lib
    template, paths, _sets = hashed_plate(tmp_path, 6, 52)
    monkeypatch.setenv("SCG_TEST_RANDOM_TAG_BITS", "0")
    with pytest.raises(sc.ScgError, match=r"collided with other keys in all 4 hash rounds") as e:
        sc.count_random_barcodes_files(paths, template, 0, 0, True, 1, devices=[0])
    assert e.value.code == _lib.SCG_ERR_UNSUPPORTED


# ---- late fall-back: a file that turns unusual after counting began ----------------------------------------------------
N_READS = 3000
MID = N_READS // 2


@pytest.fixture(params=["device_scan", "host_parse"])
def scan(request, monkeypatch):
    """Who looks at plain files first: the device record scan (default) or only the host parsers ($SCG_DEVICE_SCAN=0)."""
    if request.param == "host_parse":
        monkeypatch.setenv("SCG_DEVICE_SCAN", "0")
    monkeypatch.setenv("SCG_FASTQ_PIECE_KB", "1")
    monkeypatch.setenv("SCG_HOST_THREADS", "3")
    return request.param


def late_design(seed):
    """Reads for a file with a flaw at record MID: `early` occurs only before the flaw (the windows counted before the
    fall-back hold it, the restart counts it again), `late` only behind it."""
    rng = random.Random(seed)
    keys = [gen.rand_seq(rng, 10) for _ in range(40)]
    early, late = "AAAACCCCGG", "GGTTAACCAA"
    reads = [r if len(r) >= 2 else r + "AC" for r in reads_of(rng, T_EQUAL, keys, N_READS)]
    for i in (5, 400, 1200):
        reads[i] = construct(rng, T_EQUAL, early)
    for i in (1600, 2900):
        reads[i] = construct(rng, T_EQUAL, late, rev=True)
    return reads, early, late


def test_late_multiline_file(sc, oracle, gpu, tmp_path, scan):
    rng = random.Random(61)
    reads, early, late = late_design(62)
    keys = [gen.rand_seq(rng, 10) for _ in range(30)]
    sets = [reads_of(rng, T_EQUAL, keys, 800), reads, reads_of(rng, T_EQUAL, keys, 500)]
    paths = [gen.write_flawed_fastq(str(tmp_path / f"m{i}.fastq"), r, {MID: "multiline"} if i == 1 else {}) for i, r in enumerate(sets)]
    parsed = [oracle.parse_fastq(p) for p in paths]
    exp = expected(oracle, parsed, T_EQUAL, 2, 1, True)
    got = sc.count_random_barcodes_files(paths, T_EQUAL, 2, 1, True, 1, devices=[0])
    check(got, exp)
    keys_out, matrix, _totals = got
    assert matrix[keys_out.index(early)].tolist() == [0, 3, 0] and matrix[keys_out.index(late)].tolist() == [0, 2, 0]


def test_late_malformed_file_fails_the_call(sc, oracle, gpu, tmp_path, scan):
    """The malformed file, second of three, fails the call with the reference's error for it.  Its own key -- seen only in
    the pass that was abandoned -- is gone with it: the next call, on the good files, is exact."""
    from oracle.pyoracle import OracleError
    from screencounter_amd import _lib
    rng = random.Random(71)
    reads, early, _late = late_design(72)
    keys = [gen.rand_seq(rng, 10) for _ in range(30)]
    sets = [reads_of(rng, T_EQUAL, keys, 800), reads, reads_of(rng, T_EQUAL, keys, 500)]
    paths = [gen.write_flawed_fastq(str(tmp_path / f"b{i}.fastq"), r, {MID: "malformed"} if i == 1 else {}) for i, r in enumerate(sets)]
    with pytest.raises(OracleError) as ref:
        oracle.parse_fastq(paths[1])
    with pytest.raises(sc.ScgError) as e:
        sc.count_random_barcodes_files(paths, T_EQUAL, 2, 1, True, 1, devices=[0])
    assert (e.value.code, str(e.value)) == (_lib.SCG_ERR_IO, str(ref.value))
    with pytest.raises(sc.ScgError) as one:
        sc.count_random_barcodes(paths[1], T_EQUAL, 2, 1, True, 1)
    assert (e.value.code, str(e.value)) == (one.value.code, str(one.value))
    good = [paths[0], paths[2]]
    got = sc.count_random_barcodes_files(good, T_EQUAL, 2, 1, True, 1, devices=[0])
    check(got, expected(oracle, [sets[0], sets[2]], T_EQUAL, 2, 1, True))
    assert early not in got[0]


# ---- a base the reverse strand cannot complement ---------------------------------------------------------------------
def test_unknown_base_on_the_reverse_strand(sc, oracle, gpu, tmp_path, five):
    from screencounter_amd import _lib
    paths, sets = five
    rng = random.Random(81)
    bad = list(sets[2])
    for at, base in ((150, "R"), (600, "Y")):
        read = gen.rc(gen.fill_template(T_EQUAL, [gen.rand_seq(rng, 10)]))
        bad[at] = read[:10] + base + read[11:]               # (equal flanks: the region starts at 6 on both strands)
    bad_path = write_plain(tmp_path / "bad.fastq", bad)
    with pytest.raises(sc.ScgError) as one:
        sc.count_random_barcodes(bad_path, T_EQUAL, 2, 0, True, 1)
    assert (one.value.code, str(one.value)) == (_lib.SCG_ERR_INVALID, "cannot complement unknown base 'R'")
    with pytest.raises(sc.ScgError) as many:
        sc.count_random_barcodes_files(paths[:2] + [bad_path] + paths[3:], T_EQUAL, 2, 0, True, 1)
    assert (many.value.code, str(many.value)) == (one.value.code, str(one.value))
    rest = paths[:2] + paths[3:]
    check(sc.count_random_barcodes_files(rest, T_EQUAL, 2, 0, True, 1), expected(oracle, sets[:2] + sets[3:], T_EQUAL, 2, 0, True))
