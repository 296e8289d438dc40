"""Files that turn unusual after counting began.

Every file entry ends in the reference-exact sequential reader when the faster readers meet something they do not handle:
a multi-line record (legal, FastqReader.hpp:66-84), a record longer than a parser window, or a malformed record (the
reference's error).  When that happens late, after the host-parsed path (ParallelFastq, scg_fastq.cpp) has counted some
windows, everything those windows added must be gone before the re-read: dense counters, the combinations of sparse mode
(the plan's map and the runs of the batches still in flight), totals, the random entry's tally.  The reference's counts do not
depend on how a file is chunked (process_data.hpp:115-124); a late fall-back is just one more chunking.

Tiny parser pieces ($SCG_FASTQ_PIECE_KB of 1 or 7 with 3 host threads) put tens of windows before a flaw in the middle or at
the end of a file of a few thousand reads.  Every entry runs with the device record scan (it declines these files first) and
with the host parsers alone, and every handler with a combination grid both dense and sparse ($SCG_DENSE_CELLS=0).  The
expectation is always the oracle applied to the oracle's own parse of the written file."""
import gzip
import os
import random

import numpy as np
import pytest

from tests import gen

pytestmark = pytest.mark.gpu

N_READS = 3000
HOST_THREADS = 3

T_SINGLE = "ACGTACGA" + "-" * 12 + "TGCATGCA"
T_COMBO = "AGCTTA" + "-" * 6 + "GGTACA" + "-" * 5 + "CCATGA"
T_RANDOM = "GATCCA" + "-" * 10 + "TTGCAG"          # equal flanks: the reverse strand's region sits at the forward offset
T_MATE1 = "CAGT" + "-" * 10 + "GGA"
T_MATE2 = "TTAC" + "-" * 9 + "CCT"

# (name, flaws of mate 1, flaws of mate 2 (paired files only), $SCG_FASTQ_PIECE_KB); positions as record indices
LAST = N_READS - 1
MID = N_READS // 2
SINGLE_SCENARIOS = [
    ("multiline@first", {0: "multiline"}, 7),
    ("multiline@middle", {MID: "multiline"}, 1),
    ("multiline@last", {LAST: "multiline"}, 7),
    ("multiline@several", {N_READS // 3: "multiline", 2 * N_READS // 3: "multiline", LAST: "multiline"}, 1),
    ("oversized@middle", {MID: "oversized"}, 1),
    ("malformed@middle", {MID: "malformed"}, 7),
    ("multiline+malformed@last", {N_READS // 4: "multiline", LAST: "malformed"}, 1),
]
PAIRED_SCENARIOS = [
    ("mate1:multiline@first", {0: "multiline"}, {}, 7),
    ("mate2:multiline@middle", {}, {MID + 7: "multiline"}, 1),
    ("mate1:multiline@third,mate2:multiline@last", {N_READS // 3: "multiline"}, {LAST: "multiline"}, 7),
    ("mate2:oversized@middle", {}, {MID + 3: "oversized"}, 1),
    ("mate2:malformed@last", {}, {LAST: "malformed"}, 7),
]


def fill(rng, template, inserts, rev=False):
    read = gen.rand_seq(rng, rng.randint(0, 10)) + gen.mutate(rng, gen.fill_template(template, inserts), 0.01, 0.003, 0.0) + \
        gen.rand_seq(rng, rng.randint(0, 10))
    return gen.rc(read) if rev else read


def at_least_two(reads):
    """(a multi-line record splits its sequence over two non-empty lines)"""
    return [r if len(r) >= 2 else r + "AC" for r in reads]


def single_end_design(seed=101):
    """One read set for all single-end entries: reads of T_COMBO carry a (row, column) of two pools that also serve as the
    valid combinations of countDualBarcodesSingleEnd (row i = (pool0[i], pool1[i]), other pairs invalid); reads of T_SINGLE
    one barcode of `single`; reads of T_RANDOM an arbitrary variable region."""
    rng = random.Random(seed)
    single = gen.make_pool(rng, 60, 12, "ACGT", min_dist=3)
    p0 = gen.make_pool(rng, 50, 6, "ACGT", min_dist=2)
    p1 = gen.make_pool(rng, 50, 5, "ACGT", min_dist=2)
    variable = [gen.rand_seq(rng, 10) for _ in range(40)]
    reads = []
    for _ in range(N_READS):
        u, rev = rng.random(), rng.random() < 0.5
        if u < 0.3:
            reads.append(fill(rng, T_SINGLE, [rng.choice(single)], rev))
        elif u < 0.5:
            i = rng.randrange(50)
            reads.append(fill(rng, T_COMBO, [p0[i], p1[i]], rev))
        elif u < 0.7:
            reads.append(fill(rng, T_COMBO, [rng.choice(p0), rng.choice(p1)], rev))
        elif u < 0.92:
            reads.append(fill(rng, T_RANDOM, [rng.choice(variable)], rev))
        else:
            reads.append(gen.rand_seq(rng, rng.randint(0, 60)))
    return dict(single=single, pool0=p0, pool1=p1, reads=at_least_two(reads))


def paired_design(seed=202):
    """Mates of T_MATE1 / T_MATE2; 50 valid pairs (pool1[i], pool2[i]) drawn from 20 x 20 distinct barcodes."""
    rng = random.Random(seed)
    u1 = gen.make_pool(rng, 20, 10, "ACGT", min_dist=3)
    u2 = gen.make_pool(rng, 20, 9, "ACGT", min_dist=3)
    pairs = rng.sample([(a, b) for a in u1 for b in u2], 50)
    reads1, reads2 = [], []
    for _ in range(N_READS):
        u = rng.random()
        if u < 0.08:
            a, b = gen.rand_seq(rng, rng.randint(0, 40)), gen.rand_seq(rng, rng.randint(0, 40))
        else:
            x, y = rng.choice(pairs) if u < 0.75 else (rng.choice(u1), rng.choice(u2))
            a, b = fill(rng, T_MATE1, [x]), fill(rng, T_MATE2, [y], rev=True)
        reads1.append(a)
        reads2.append(b)
    return dict(pool1=[a for a, _ in pairs], pool2=[b for _, b in pairs], u1=u1, u2=u2,
                reads1=at_least_two(reads1), reads2=at_least_two(reads2))


SINGLE_END = single_end_design()
PAIRED = paired_design()


def write_single(path, scenario):
    _name, flaws, _kb = scenario
    return gen.write_flawed_fastq(path, SINGLE_END["reads"], flaws, seed=len(flaws))


def write_paired(dirpath, scenario):
    _name, flaws1, flaws2, _kb = scenario
    return (gen.write_flawed_fastq(os.path.join(dirpath, "m1.fastq"), PAIRED["reads1"], flaws1, seed=1),
            gen.write_flawed_fastq(os.path.join(dirpath, "m2.fastq"), PAIRED["reads2"], flaws2, seed=2))


# ---- the entries, and what the oracle says they return, as plain lists and numbers -------------------------------------
def _l(a):
    return np.asarray(a).tolist()


def _fields(d, *keys):
    return tuple(_l(d[k]) if isinstance(d[k], np.ndarray) else d[k] for k in keys)


S, P = SINGLE_END, PAIRED
POOLS = [S["pool0"], S["pool1"]]


def got_single(sc, p):
    c, t = sc.count_single_barcodes(p, T_SINGLE, 2, S["single"], 1, True, 1)
    return _l(c), t


def exp_single(o, r):
    c, t = o.count_single(r, T_SINGLE, 2, S["single"], 1, True)
    return _l(c), t


def got_combo(sc, p):
    i, f, t = sc.count_combo_barcodes_single(p, T_COMBO, 2, POOLS, 1, True, 1)
    return _l(i), _l(f), t


def exp_combo(o, r):
    i, f, t = o.count_combo(r, T_COMBO, 2, S["pool0"], S["pool1"], 1, True)
    return _l(i), _l(f), t


def got_dual_single_end(sc, p):
    c, t = sc.count_dual_barcodes_single_end(p, T_COMBO, POOLS, 2, 1, True, False, 1)
    return _l(c), t


def exp_dual_single_end(o, r):
    c, t = o.count_dual_single_end(r, T_COMBO, 2, POOLS, 1, True)
    return _l(c), t


def got_dual_single_end_diag(sc, p):
    c, (i, f), t = sc.count_dual_barcodes_single_end(p, T_COMBO, POOLS, 2, 1, True, True, 1)
    return _l(c), _l(i), _l(f), t


def exp_dual_single_end_diag(o, r):
    return _fields(o.count_dual_single_end_diag(r, T_COMBO, 2, POOLS, 1, True), "counts", "indices", "freq", "total")


def got_random(sc, p):
    (seqs, freq), t = sc.count_random_barcodes(p, T_RANDOM, 2, 1, True, 1)
    return dict(zip(seqs, _l(freq))), t


def exp_random(o, r):
    return o.count_random(r, T_RANDOM, 2, 1, True)


MATES = (T_MATE1, False, 1, P["pool1"], T_MATE2, True, 1, P["pool2"])


def got_dual(sc, p1, p2):
    c, t = sc.count_dual_barcodes(p1, T_MATE1, False, 1, P["pool1"], p2, T_MATE2, True, 1, P["pool2"], False, True, False, 1)
    return _l(c), t


def exp_dual(o, r1, r2):
    c, t = o.count_dual(r1, r2, *MATES, False, True)
    return _l(c), t


def got_dual_diag(sc, p1, p2):
    c, (i, f), t, b1, b2 = sc.count_dual_barcodes(p1, T_MATE1, False, 1, P["pool1"], p2, T_MATE2, True, 1, P["pool2"], False, True, True, 1)
    return _l(c), _l(i), _l(f), t, b1, b2


def exp_dual_diag(o, r1, r2):
    return _fields(o.count_dual_diag(r1, r2, *MATES, False, True), "counts", "indices", "freq", "total", "barcode1_only", "barcode2_only")


def got_combo_paired(sc, p1, p2):
    i, f, t, b1, b2 = sc.count_combo_barcodes_paired(p1, T_MATE1, False, 1, P["u1"], p2, T_MATE2, True, 1, P["u2"], False, True, 1)
    return _l(i), _l(f), t, b1, b2


def exp_combo_paired(o, r1, r2):
    d = o.count_combo_paired(r1, r2, T_MATE1, False, 1, P["u1"], T_MATE2, True, 1, P["u2"], False, True)
    return _fields(d, "indices", "freq", "total", "barcode1_only", "barcode2_only")


SINGLE_ENTRIES = {name: (globals()["got_" + name], globals()["exp_" + name])
                  for name in ("single", "combo", "dual_single_end", "dual_single_end_diag", "random")}
PAIRED_ENTRIES = {name: (globals()["got_" + name], globals()["exp_" + name]) for name in ("dual", "dual_diag", "combo_paired")}
GRID = {"combo", "dual_single_end_diag", "dual_diag", "combo_paired"}      # the handlers with a combination grid (scg_plan.cpp)


def expected_single(oracle, path, entry):
    """("ok", result) or ("error", message) -- the oracle on the oracle's parse of the file."""
    from oracle.pyoracle import OracleError
    try:
        return "ok", SINGLE_ENTRIES[entry][1](oracle, oracle.parse_fastq(path))
    except OracleError as e:
        return "error", str(e)


def expected_paired(oracle, p1, p2, entry):
    from oracle.pyoracle import OracleError
    try:
        return "ok", PAIRED_ENTRIES[entry][1](oracle, oracle.parse_fastq(p1), oracle.parse_fastq(p2))
    except OracleError as e:
        return "error", str(e)


def outcome(fn):
    from screencounter_amd import _lib
    try:
        return "ok", fn()
    except _lib.ScgError as e:
        assert e.code == _lib.SCG_ERR_IO, (e.code, str(e))
        return "error", str(e)


def describe(got, exp):
    """How far apart two results are: for counts, the sums and the largest difference."""
    if got[0] != exp[0] or got[0] == "error":
        return f"got {got!r:.300}, expected {exp!r:.300}"
    parts = []
    for k, (g, e) in enumerate(zip(got[1], exp[1])):
        if g == e:
            continue
        if isinstance(g, dict):
            parts.append(f"[{k}] sum {sum(g.values())} vs {sum(e.values())}")
        elif isinstance(g, list) and g and not isinstance(g[0], list):
            parts.append(f"[{k}] sum {sum(g)} vs {sum(e)} (len {len(g)} vs {len(e)})")
        else:
            parts.append(f"[{k}] {g!r:.80} vs {e!r:.80}")
    return "; ".join(parts)


def check(got, exp):
    assert got == exp, describe(got, exp)


@pytest.fixture(params=["device_scan", "host_parse"])
def scan(request, monkeypatch):
    """Who looks at plain files first: the device record scan (default) or only the host parsers ($SCG_DEVICE_SCAN=0)."""
    if request.param == "host_parse":
        monkeypatch.setenv("SCG_DEVICE_SCAN", "0")
    return request.param


def grid_storage(monkeypatch, storage):
    monkeypatch.setenv("SCG_HOST_THREADS", str(HOST_THREADS))
    if storage == "sparse":
        monkeypatch.setenv("SCG_DENSE_CELLS", "0")
    else:
        monkeypatch.delenv("SCG_DENSE_CELLS", raising=False)


def entry_storage(entries):
    return [(e, s) for e in entries for s in (("dense", "sparse") if e in GRID else ("dense",))]


@pytest.mark.parametrize("scenario", SINGLE_SCENARIOS, ids=[s[0] for s in SINGLE_SCENARIOS])
@pytest.mark.parametrize("entry,storage", entry_storage(SINGLE_ENTRIES))
def test_single_end_entries(sc, oracle, gpu, tmp_path, monkeypatch, scan, entry, storage, scenario):
    grid_storage(monkeypatch, storage)
    monkeypatch.setenv("SCG_FASTQ_PIECE_KB", str(scenario[2]))
    path = write_single(str(tmp_path / "r.fastq"), scenario)
    exp = expected_single(oracle, path, entry)
    check(outcome(lambda: SINGLE_ENTRIES[entry][0](sc, path)), exp)


@pytest.mark.parametrize("scenario", PAIRED_SCENARIOS, ids=[s[0] for s in PAIRED_SCENARIOS])
@pytest.mark.parametrize("entry,storage", entry_storage(PAIRED_ENTRIES))
def test_paired_entries(sc, oracle, gpu, tmp_path, monkeypatch, scan, entry, storage, scenario):
    grid_storage(monkeypatch, storage)
    monkeypatch.setenv("SCG_FASTQ_PIECE_KB", str(scenario[3]))
    p1, p2 = write_paired(str(tmp_path), scenario)
    exp = expected_paired(oracle, p1, p2, entry)
    check(outcome(lambda: PAIRED_ENTRIES[entry][0](sc, p1, p2)), exp)


@pytest.mark.parametrize("devices", ["0,0", "0,0,0"])
def test_several_plans_of_one_call(sc, oracle, gpu, tmp_path, monkeypatch, scan, devices):
    """Several plans (one card listed more than once): the fall-back counts on the first plan after every plan was reset."""
    monkeypatch.setenv("SCG_DEVICES", devices)
    for storage in ("dense", "sparse"):
        grid_storage(monkeypatch, storage)
        for scenario in (SINGLE_SCENARIOS[1], SINGLE_SCENARIOS[2], SINGLE_SCENARIOS[4]):
            monkeypatch.setenv("SCG_FASTQ_PIECE_KB", str(scenario[2]))
            path = write_single(str(tmp_path / "r.fastq"), scenario)
            for entry in ("combo", "dual_single_end_diag"):
                check(outcome(lambda: SINGLE_ENTRIES[entry][0](sc, path)), expected_single(oracle, path, entry))
        for scenario in PAIRED_SCENARIOS[1:4]:
            monkeypatch.setenv("SCG_FASTQ_PIECE_KB", str(scenario[3]))
            p1, p2 = write_paired(str(tmp_path), scenario)
            for entry in PAIRED_ENTRIES:
                check(outcome(lambda: PAIRED_ENTRIES[entry][0](sc, p1, p2)), expected_paired(oracle, p1, p2, entry))


@pytest.mark.parametrize("form", ["bgzf", "gzip"])
def test_compressed_forms_of_the_same_text(sc, oracle, gpu, tmp_path, monkeypatch, scan, form):
    """The flawed text as BGZF and as ordinary gzip: the device inflater and scan decline it, then the host readers; the
    plans are reset by those fall-backs (the ladders of csrc/scg_files.cpp) before the sequential reader takes the file."""
    monkeypatch.setenv("SCG_HOST_THREADS", str(HOST_THREADS))
    for storage in ("dense", "sparse"):
        grid_storage(monkeypatch, storage)
        for scenario in (SINGLE_SCENARIOS[1], SINGLE_SCENARIOS[2], SINGLE_SCENARIOS[5]):
            monkeypatch.setenv("SCG_FASTQ_PIECE_KB", str(scenario[2]))
            plain = write_single(str(tmp_path / "r.fastq"), scenario)
            text = open(plain, "rb").read()
            path = str(tmp_path / "r.fastq.gz")
            if form == "bgzf":
                gen.write_bgzf(path, text, block=5000)
            else:
                with gzip.open(path, "wb") as f:
                    f.write(text)
            for entry in ("single", "combo"):
                check(outcome(lambda: SINGLE_ENTRIES[entry][0](sc, path)), expected_single(oracle, plain, entry))


def test_multi_file_entries(sc, oracle, gpu, tmp_path, monkeypatch, scan):
    """Three files, only the middle one flawed late: every column equals a one-file call and the oracle."""
    monkeypatch.setenv("SCG_HOST_THREADS", str(HOST_THREADS))
    monkeypatch.setenv("SCG_FASTQ_PIECE_KB", "1")
    reads = SINGLE_END["reads"]
    thirds = [reads[:1000], reads[1000:2500], reads[2500:]]
    mid = [{}, {700: "multiline"}, {}]
    files = [gen.write_flawed_fastq(str(tmp_path / f"s{i}.fastq"), r, f) for i, (r, f) in enumerate(zip(thirds, mid))]
    m1, m2 = PAIRED["reads1"], PAIRED["reads2"]
    pthirds = [(m1[:900], m2[:900]), (m1[900:2400], m2[900:2400]), (m1[2400:], m2[2400:])]
    pfiles1 = [gen.write_flawed_fastq(str(tmp_path / f"a{i}.fastq"), r1, {}) for i, (r1, _) in enumerate(pthirds)]
    pfiles2 = [gen.write_flawed_fastq(str(tmp_path / f"b{i}.fastq"), r2, {1000: "multiline"} if i == 1 else {})
               for i, (_, r2) in enumerate(pthirds)]
    for storage in ("dense", "sparse"):
        grid_storage(monkeypatch, storage)
        monkeypatch.setenv("SCG_FASTQ_PIECE_KB", "1")
        for devices in (None, [0, 0]):
            mat, tot = sc.count_single_barcodes_files(files, T_SINGLE, 2, S["single"], 1, True, 1, devices)
            for c, f in enumerate(files):
                assert (mat[:, c].tolist(), tot[c]) == SINGLE_ENTRIES["single"][0](sc, f) == expected_single(oracle, f, "single")[1], (devices, c)
            per = sc.count_combo_barcodes_single_files(files, T_COMBO, 2, POOLS, 1, True, 1, devices)
            for c, (f, (idx, freq, total)) in enumerate(zip(files, per)):
                got = (_l(idx), _l(freq), total)
                assert got == SINGLE_ENTRIES["combo"][0](sc, f), (storage, devices, c)
                check(("ok", got), expected_single(oracle, f, "combo"))
            mat, tot = sc.count_dual_barcodes_files(pfiles1, T_MATE1, False, 1, P["pool1"], pfiles2, T_MATE2, True, 1, P["pool2"],
                                                    False, True, 1, devices)
            for c, (f1, f2) in enumerate(zip(pfiles1, pfiles2)):
                got = (mat[:, c].tolist(), tot[c])
                assert got == PAIRED_ENTRIES["dual"][0](sc, f1, f2), (devices, c)
                check(("ok", got), expected_paired(oracle, f1, f2, "dual"))


def unknown_base_read(rng, base):
    """A reverse-strand read of T_RANDOM whose variable region holds `base`, which the reference cannot complement."""
    region = gen.rand_seq(rng, 10)
    read = gen.rc(gen.fill_template(T_RANDOM, [region]))
    at = 6 + 4                                       # (T_RANDOM's flanks are equal: the region is at the forward offset)
    return read[:at] + base + read[at + 1:]


@pytest.mark.parametrize("piece_kb", [1, 7])
def test_random_entry_reports_the_first_unknown_base(sc, oracle, gpu, tmp_path, monkeypatch, scan, piece_kb):
    """countRandomBarcodes stops at the first read (in file order) whose reverse-strand region it cannot complement -- in a
    window counted before the late flaw, or in the part the sequential reader counts after it."""
    monkeypatch.setenv("SCG_HOST_THREADS", str(HOST_THREADS))
    monkeypatch.setenv("SCG_FASTQ_PIECE_KB", str(piece_kb))
    rng = random.Random(303)
    reads = list(SINGLE_END["reads"])
    flaw = 2000
    for name, first, second in (("before", 700, 2600), ("after", 2300, 2700)):
        r = list(reads)
        r[first] = unknown_base_read(rng, "R")
        r[second] = unknown_base_read(rng, "Y")
        path = gen.write_flawed_fastq(str(tmp_path / f"{name}.fastq"), r, {flaw: "multiline"})
        exp = expected_single(oracle, path, "random")
        assert exp == ("error", "cannot complement unknown base 'R'"), (name, exp)
        from screencounter_amd import _lib
        with pytest.raises(_lib.ScgError) as e:
            SINGLE_ENTRIES["random"][0](sc, path)
        assert e.value.code == _lib.SCG_ERR_INVALID and str(e.value) == exp[1], name


def test_against_kaori_where_built(sc, oracle, gpu, tmp_path, monkeypatch):
    """A few late-flaw files read by kaori itself (oracle/_ref/libkaori_ref.so, where it was built): the oracle's parse and
    counts agree with it, and so do the entries."""
    from oracle.pyoracle import KaoriRef, OracleError
    monkeypatch.setenv("SCG_HOST_THREADS", str(HOST_THREADS))
    monkeypatch.setenv("SCG_DENSE_CELLS", "0")
    kaori = KaoriRef() if KaoriRef.available() else None
    for scenario in (SINGLE_SCENARIOS[2], SINGLE_SCENARIOS[4], SINGLE_SCENARIOS[6]):
        monkeypatch.setenv("SCG_FASTQ_PIECE_KB", str(scenario[2]))
        path = write_single(str(tmp_path / "r.fastq"), scenario)
        for entry in ("single", "combo", "random"):
            exp = expected_single(oracle, path, entry)
            check(outcome(lambda: SINGLE_ENTRIES[entry][0](sc, path)), exp)
            if kaori is None:
                continue
            try:
                if entry == "single":
                    c, t = kaori.count_single(path, T_SINGLE, 2, S["single"], 1, True)
                    ref = ("ok", (_l(c), t))
                elif entry == "combo":
                    i, f, t = kaori.count_combo(path, T_COMBO, 2, S["pool0"], S["pool1"], 1, True)
                    ref = ("ok", (_l(i), _l(f), t))
                else:
                    ref = ("ok", kaori.count_random(path, T_RANDOM, 2, 1, True))
            except OracleError as e:
                ref = ("error", str(e))
            check(ref, exp)
