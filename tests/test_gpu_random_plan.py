"""Random-barcode plans (Plan.random / read_random): the countRandomBarcodes tally kept in HBM across batches, against the
oracle, the file entry point and plain Python counters.

The oracle upper-cases the byte it names in "cannot complement unknown base 'X'"; the reference (kaori/utils.hpp:117) and
the file entry name the byte as it is in the read.  Messages are therefore compared exactly with the file entry and
without regard to case with the oracle.
"""
import collections
import random

import numpy as np
import pytest

from tests import gen

pytestmark = pytest.mark.gpu


def count_batches(sc, plan, batches, device, fixed=False, stream=None):
    for reads in batches:
        if fixed:
            n = len(reads)
            width = len(reads[0]) if n else 0
            if n and width:
                seqs, _ = sc.upload_reads(reads, device)
                plan.count(seqs, fixed_len=width, n_reads=n, stream=stream)
            else:
                seqs, offs = sc.upload_reads(reads, device)
                plan.count(seqs, offs, stream=stream)
        else:
            seqs, offs = sc.upload_reads(reads, device)
            plan.count(seqs, offs, stream=stream)


def random_split(rng, reads):
    k = rng.randint(1, 4)
    cuts = sorted(rng.randint(0, len(reads)) for _ in range(k - 1))
    bounds = [0] + cuts + [len(reads)]
    return [reads[bounds[i]:bounds[i + 1]] for i in range(k)]


def by_length(reads):
    """Fixed-length batches: the reads grouped by length (stable), one batch per length."""
    groups = collections.OrderedDict()
    for r in reads:
        groups.setdefault(len(r), []).append(r)
    return list(groups.values())


def plan_result(sc, case, batches, device, fixed=False):
    with sc.Plan.random(case["template"], case["strand"], case["mismatches"], case["use_first"]) as plan:
        count_batches(sc, plan, batches, device, fixed=fixed)
        try:
            (seqs, freq), total = plan.read_random()
        except sc.ScgError as e:
            return e
    return seqs, freq, total


def oracle_result(oracle, reads, case):
    from oracle.pyoracle import OracleError
    try:
        return oracle.count_random(reads, case["template"], case["strand"], case["mismatches"], case["use_first"])
    except OracleError as e:
        return e


@pytest.mark.parametrize("seed", range(6))
def test_random_plan_matches_oracle_and_file_entry(sc, oracle, gpu, seed, tmp_path):
    from oracle.pyoracle import write_fastq
    rng = random.Random(9100 + seed)
    for it in range(15):
        case = gen.random_random_barcode_case(rng, sizes=(1, 40, 400))
        reads = case["reads"]
        # ragged batches, in file order
        exp = oracle_result(oracle, reads, case)
        got = plan_result(sc, case, random_split(rng, reads), gpu)
        fq = str(tmp_path / f"r{it}.fastq")
        write_fastq(fq, reads)
        try:
            file_res = sc.count_random_barcodes(fq, case["template"], case["strand"], case["mismatches"], case["use_first"], 1)
        except sc.ScgError as e:
            file_res = e
        if isinstance(exp, Exception):
            assert isinstance(got, sc.ScgError), (case, got)
            assert str(got).upper() == str(exp).upper(), (str(got), str(exp))
            assert isinstance(file_res, sc.ScgError) and str(got) == str(file_res), (str(got), str(file_res))
        else:
            assert not isinstance(got, Exception), (case, got)
            seqs, freq, total = got
            assert total == exp[1] and seqs == sorted(seqs) and dict(zip(seqs, freq.tolist())) == exp[0], (case, exp, got)
            (fseqs, ffreq), ftotal = file_res
            assert fseqs == seqs and np.array_equal(ffreq, freq) and ftotal == total
        # fixed-length batches (reads grouped by length: the oracle sees the same order)
        fixed_reads = [r for b in by_length(reads) for r in b]
        exp = oracle_result(oracle, fixed_reads, case)
        got = plan_result(sc, case, by_length(reads), gpu, fixed=True)
        if isinstance(exp, Exception):
            assert isinstance(got, sc.ScgError) and str(got).upper() == str(exp).upper(), (str(got), str(exp))
        else:
            seqs, freq, total = got
            assert total == exp[1] and dict(zip(seqs, freq.tolist())) == exp[0] and seqs == sorted(seqs), (case, exp, got)


def _construct_reads(rng, template, keys, n, reverse_share):
    reads = []
    for _ in range(n):
        k = rng.choice(keys)
        core = template.replace("-" * template.count("-"), k) if template.count("-") else template
        read = gen.rand_seq(rng, rng.randint(0, 6)) + core + gen.rand_seq(rng, rng.randint(0, 6))
        if rng.random() < reverse_share:
            read = gen.rc(read)
        reads.append(read)
    return reads


@pytest.mark.parametrize("vlen", [1, 30, 31, 32, 33, 64, 65, 200, 255])
def test_random_plan_key_lengths_and_alphabets(sc, oracle, gpu, vlen):
    """Packed (pure ACGT up to 31 bases) and hashed keys (longer, N, lower case, IUPAC), both strands, up to the longest
    region a 256-base template holds."""
    rng = random.Random(9500 + vlen)
    template = ("G" + "-" * vlen) if vlen >= 250 else ("ACGTAC" + "-" * vlen + "TTGCAG")
    assert len(template) <= 256
    for alphabet, reverse_share in (("ACGT", 0.5), ("ACGTN", 0.5), ("ACGTacgtn", 0.5), ("ACGTRYKM", 0.0), ("ACGTNRY", 0.0)):
        keys = sorted({gen.rand_seq(rng, vlen, alphabet) for _ in range(12)})
        reads = _construct_reads(rng, template, keys, 300, reverse_share)
        case = dict(template=template, strand=2 if reverse_share else 0, mismatches=0, use_first=True)
        exp = oracle_result(oracle, reads, case)
        got = plan_result(sc, case, random_split(rng, reads), gpu)
        assert not isinstance(exp, Exception), exp
        assert not isinstance(got, Exception), got
        seqs, freq, total = got
        assert total == exp[1] == len(reads) and dict(zip(seqs, freq.tolist())) == exp[0] and seqs == sorted(seqs), (alphabet, vlen)


def _fixed_reads(keys: np.ndarray, left: bytes, right: bytes) -> np.ndarray:
    n = keys.shape[0]
    out = np.empty((n, len(left) + keys.shape[1] + len(right)), dtype=np.uint8)
    out[:, :len(left)] = np.frombuffer(left, dtype=np.uint8)
    out[:, len(left):len(left) + keys.shape[1]] = keys
    out[:, len(left) + keys.shape[1]:] = np.frombuffer(right, dtype=np.uint8)
    return out


def _count_fixed(sc, plan, rows: np.ndarray, n_batches: int, gpu):
    import torch
    for part in np.array_split(rows, n_batches):
        t = torch.from_numpy(np.ascontiguousarray(part).reshape(-1)).to(gpu)
        plan.count(t, fixed_len=rows.shape[1], n_reads=part.shape[0])


def test_random_plan_growth(sc, gpu):
    """~2 M distinct 20-mers plus hot keys, from the initial 2^16-slot table through several doublings."""
    rng = np.random.default_rng(11)
    acgt = np.frombuffer(b"ACGT", dtype=np.uint8)
    distinct = acgt[rng.integers(0, 4, size=(2_000_000, 20))]
    hot = acgt[rng.integers(0, 4, size=(3, 20))]
    keys = np.concatenate([distinct, np.repeat(hot, [50_000, 20_000, 7], axis=0)])
    keys = keys[rng.permutation(keys.shape[0])]
    rows = _fixed_reads(keys, b"ACGTAC", b"TTGCAG")
    with sc.Plan.random("ACGTAC" + "-" * 20 + "TTGCAG", 0) as plan:
        _count_fixed(sc, plan, rows, 7, gpu)
        (seqs, freq), total = plan.read_random()
    uniq, counts = np.unique(keys.view("S20").ravel(), return_counts=True)
    assert total == keys.shape[0]
    assert len(seqs) == uniq.size
    assert seqs == [u.decode() for u in uniq]
    assert np.array_equal(freq, counts.astype(np.int32))


def test_random_plan_skew(sc, gpu):
    """10^6 reads on 3 keys, both strands: exact counts."""
    rng = np.random.default_rng(12)
    keys = [b"ACGTTGCAACGTTGCAAC", b"TTTTTTTTTTTTTTTTTT", b"GATTACAGATTACAGATT"]
    which = rng.choice(3, size=1_000_000, p=[0.9, 0.09, 0.01])
    karr = np.stack([np.frombuffer(k, dtype=np.uint8) for k in keys])[which]
    rows = _fixed_reads(karr, b"CCAGTC", b"GGATCA")
    rev = rng.random(rows.shape[0]) < 0.3
    comp = np.zeros(256, dtype=np.uint8)
    for a, b in zip(b"ACGT", b"TGCA"):
        comp[a] = b
    rows[rev] = comp[rows[rev][:, ::-1]]
    with sc.Plan.random("CCAGTC" + "-" * 18 + "GGATCA", 2) as plan:
        _count_fixed(sc, plan, rows, 3, gpu)
        (seqs, freq), total = plan.read_random()
    exp = {k.decode(): int((which == i).sum()) for i, k in enumerate(keys)}
    assert total == rows.shape[0]
    assert dict(zip(seqs, freq.tolist())) == exp and seqs == sorted(seqs)


def _hashed_case(n_keys, seed):
    rng = random.Random(seed)
    template = "ACGTAC" + "-" * 12 + "TTGCAG"
    hashed = sorted({gen.rand_seq(rng, 12, "acgtN") for _ in range(n_keys * 3)})[:n_keys]
    packed = [gen.rand_seq(rng, 12) for _ in range(3)]
    reads = _construct_reads(rng, template, hashed + packed, 3000, 0.0)
    return template, reads


def test_random_plan_collisions_resolved(sc, oracle, gpu, monkeypatch):
    """With no hash bits in the tags every hashed key of a round collides; each round settles one key, so four hashed keys
    come out exact."""
    template, reads = _hashed_case(4, 31)
    monkeypatch.setenv("SCG_TEST_RANDOM_TAG_BITS", "0")
    case = dict(template=template, strand=0, mismatches=0, use_first=True)
    exp = oracle_result(oracle, reads, case)
    got = plan_result(sc, case, [reads[:1000], reads[1000:1700], reads[1700:]], gpu)
    seqs, freq, total = got
    assert total == exp[1] and dict(zip(seqs, freq.tolist())) == exp[0]


def test_random_plan_collisions_exhausted(sc, gpu, monkeypatch):
    """Six hashed keys against four rounds with no hash bits: read-out fails rather than return wrong counts."""
    template, reads = _hashed_case(6, 32)
    monkeypatch.setenv("SCG_TEST_RANDOM_TAG_BITS", "0")
    with sc.Plan.random(template, 0) as plan:
        count_batches(sc, plan, [reads[:1500], reads[1500:]], gpu)
        with pytest.raises(sc.ScgError, match="collided"):
            plan.read_random()


def _lifecycle_reads(seed, n=2000):
    rng = random.Random(seed)
    template = "ACGTAC" + "-" * 10 + "TTGCAG"
    keys = [gen.rand_seq(rng, 10, "ACGTn") for _ in range(40)]
    return template, _construct_reads(rng, template, keys, n, 0.5)


def test_random_plan_reset_and_read_twice(sc, oracle, gpu):
    template, reads = _lifecycle_reads(41)
    case = dict(template=template, strand=2, mismatches=0, use_first=True)
    exp = oracle_result(oracle, reads[1000:], case)
    with sc.Plan.random(template, 2) as plan:
        count_batches(sc, plan, [reads[:1000]], gpu)
        plan.reset()
        count_batches(sc, plan, [reads[1000:1500], reads[1500:]], gpu)
        first = plan.read_random()
        second = plan.read_random()
    assert first[0][0] == second[0][0] and np.array_equal(first[0][1], second[0][1]) and first[1] == second[1]
    assert first[1] == exp[1] and dict(zip(first[0][0], first[0][1].tolist())) == exp[0]


def test_random_plan_two_streams(sc, gpu):
    import torch
    template, reads = _lifecycle_reads(42, 4000)
    batches = [reads[i:i + 500] for i in range(0, len(reads), 500)]
    uploaded = [sc.upload_reads(b, gpu) for b in batches]
    torch.cuda.synchronize()
    with sc.Plan.random(template, 2) as plan:
        for s, o in uploaded:
            plan.count(s, o)
        one = plan.read_random()
    streams = [torch.cuda.Stream(), torch.cuda.Stream()]
    with sc.Plan.random(template, 2) as plan:
        for i, (s, o) in enumerate(uploaded):
            plan.count(s, o, stream=streams[i % 2])
        two = plan.read_random(stream=streams[1])
    assert one[0][0] == two[0][0] and np.array_equal(one[0][1], two[0][1]) and one[1] == two[1] == len(reads)


def test_random_plan_repeats_identical(sc, gpu):
    template, reads = _lifecycle_reads(43, 3000)
    outs = []
    for _ in range(3):
        with sc.Plan.random(template, 2) as plan:
            count_batches(sc, plan, [reads[:1234], reads[1234:]], gpu)
            (seqs, freq), total = plan.read_random()
            outs.append((seqs, freq.tolist(), total))
    assert outs[0] == outs[1] == outs[2]


def test_random_plan_empty_and_no_hit_batches(sc, gpu):
    template, reads = _lifecycle_reads(44, 500)
    with sc.Plan.random(template, 2) as plan:
        count_batches(sc, plan, [[]], gpu)
        (seqs, freq), total = plan.read_random()
        assert seqs == [] and freq.size == 0 and total == 0
        misses = ["GGGGGGGGGGGGGGGGGGGGGGGGGGGGGG", "A", ""]
        count_batches(sc, plan, [misses], gpu)
        (seqs, freq), total = plan.read_random()
        assert seqs == [] and freq.size == 0 and total == 3
        count_batches(sc, plan, [reads], gpu)
        (seqs, freq), total = plan.read_random()
        assert total == 503 and int(freq.sum()) > 0
        _, plain_total = plan.read()
        assert plain_total == 503 and plan.num_counters == 0


def test_random_plan_oversize_read_is_reported(sc, gpu):
    template, reads = _lifecycle_reads(45, 200)
    reads = reads + ["ACGTAC" + "A" * 10 + "TTGCAG" + "C" * 200]
    with sc.Plan.random(template, 2) as plan:
        seqs, offs = sc.upload_reads(reads, gpu)
        plan.count(seqs, offs, max_len=100)     # a lie: one read is 222 bases long
        with pytest.raises(sc.ScgError, match="longer than the max_len"):
            plan.read_random()


def test_random_plan_rejects_other_calls(sc, gpu):
    import torch
    with sc.Plan.random("ACGT----ACGT", 0) as plan:
        with pytest.raises(sc.ScgError):
            plan.bind_counters(torch.zeros(1, dtype=torch.int32, device=gpu))
        s, o = sc.upload_reads(["ACGTAAAAACGT"], gpu)
        with pytest.raises(sc.ScgError):
            plan.count_paired(s, s, o, o)
        with pytest.raises(ValueError):
            plan.read_combo()
