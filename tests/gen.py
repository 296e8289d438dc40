"""Random workload generators shared by the oracle fuzzers and the parity tests (test infrastructure)."""
from __future__ import annotations

import random

BASES = "ACGT"
COMP = {"A": "T", "C": "G", "G": "C", "T": "A", "N": "N", "a": "t", "c": "g", "g": "c", "t": "a", "n": "n"}
IUPAC = "RYSWKMBDHVN"


def rc(s: str) -> str:
    return "".join(COMP.get(c, "N") for c in reversed(s))


def rand_seq(rng: random.Random, n: int, alphabet: str = BASES) -> str:
    return "".join(rng.choice(alphabet) for _ in range(n))


def mutate(rng: random.Random, s: str, p_sub: float, p_n: float, p_lower: float) -> str:
    out = []
    for c in s:
        if rng.random() < p_sub:
            c = rng.choice([b for b in BASES if b != c.upper()])
        if rng.random() < p_n:
            c = rng.choice("NnRX.")  # any non-ACGT byte is "other" to the scanner
        if rng.random() < p_lower:
            c = c.lower()
        out.append(c)
    return "".join(out)


def make_pool(rng: random.Random, n: int, length: int, alphabet: str, min_dist: int = 1, iupac_rate: float = 0.0):
    """distinct sequences with pairwise Hamming distance >= min_dist (on the concrete bases)"""
    pool: list[str] = []
    tries = 0
    while len(pool) < n and tries < 20000:
        tries += 1
        s = rand_seq(rng, length, alphabet)
        if all(sum(a != b for a, b in zip(s, t)) >= min_dist for t in pool):
            pool.append(s)
    if iupac_rate > 0:
        pool = ["".join(rng.choice(IUPAC) if rng.random() < iupac_rate else c for c in s) for s in pool]
    return pool


def make_template(rng: random.Random, nvar: int, var_lens: list[int], flank_lo: int, flank_hi: int) -> str:
    parts = [rand_seq(rng, rng.randint(flank_lo, flank_hi))]
    for v in range(nvar):
        parts.append("-" * var_lens[v])
        lo = max(flank_lo, 1) if v < nvar - 1 else flank_lo  # keep regions separate
        parts.append(rand_seq(rng, rng.randint(lo, flank_hi)))
    t = "".join(parts)
    if rng.random() < 0.2:
        t = t.lower()
    return t


def fill_template(template: str, inserts: list[str]) -> str:
    out = []
    it = iter(inserts)
    i = 0
    while i < len(template):
        if template[i] == "-":
            j = i
            while j < len(template) and template[j] == "-":
                j += 1
            out.append(next(it))
            i = j
        else:
            out.append(template[i].upper())
            i += 1
    return "".join(out)


def concrete(rng: random.Random, s: str) -> str:
    """pick one concrete expansion of an IUPAC library string"""
    table = {"R": "AG", "Y": "CT", "S": "CG", "W": "AT", "K": "GT", "M": "AC", "B": "CGT", "D": "AGT", "H": "ACT", "V": "ACG", "N": "ACGT"}
    return "".join(rng.choice(table[c]) if c in table else c for c in s.upper())


def make_reads(rng, template, pools, n, strand, p_sub, p_n, p_lower, p_junk, pad_hi, valid_pairs=None):
    reads = []
    for _ in range(n):
        if rng.random() < p_junk:
            reads.append(rand_seq(rng, rng.randint(0, len(template) + pad_hi)))
            continue
        if valid_pairs is not None:
            raise AssertionError
        ins = [concrete(rng, rng.choice(p)) for p in pools]
        core = fill_template(template, ins)
        core = mutate(rng, core, p_sub, p_n, p_lower)
        read = rand_seq(rng, rng.randint(0, pad_hi)) + core + rand_seq(rng, rng.randint(0, pad_hi))
        if rng.random() < 0.1:  # two constructs in one read
            ins2 = [concrete(rng, rng.choice(p)) for p in pools]
            read += rand_seq(rng, rng.randint(0, 3)) + mutate(rng, fill_template(template, ins2), p_sub, p_n, p_lower)
        if strand == 1 or (strand == 2 and rng.random() < 0.5):
            read = rc(read)
        reads.append(read)
    return reads




# ---------------------------------------------------------------------------------------------
# Whole random cases (inputs only) for the three entry points and the matcher.
# ---------------------------------------------------------------------------------------------
def random_single_case(rng: random.Random, max_vlen: int = 33, sizes=(1, 30, 200), min_vlen: int = 0) -> dict:
    vlen = rng.choice([v for v in (3, 4, 6, 8, 10, 20, 33, 40, 57, 64, 65, 100, 128, 129, 200, 240) if min_vlen <= v <= max_vlen])
    alphabet = rng.choice(["AC", "ACG", BASES, BASES])
    npool = rng.choice([1, 2, 5, 20, 100])
    pool = make_pool(rng, npool, vlen, alphabet, min_dist=1, iupac_rate=rng.choice([0, 0, 0.05 if vlen <= 64 else 0.01]))
    template = make_template(rng, 1, [vlen], rng.choice([0, 1, 3]), rng.choice([4, 8, 12, 40]) if vlen <= 128 else 8)    # (templates: at most 256)
    strand = rng.choice([0, 1, 2])
    mm = rng.choice([0, 1, 1, 2, 3])
    first = rng.random() < 0.5
    reads = make_reads(rng, template, [pool], rng.choice(sizes), strand, rng.choice([0, 0.02, 0.08]), rng.choice([0, 0.01, 0.05]),
                       rng.choice([0, 0.3]), 0.1, rng.choice([0, 5, 30]))
    return dict(kind="single", template=template, strand=strand, pool=pool, mismatches=mm, use_first=first, reads=reads)


def random_combo_case(rng: random.Random, sizes=(1, 30, 200), wide: bool = False) -> dict:
    v0, v1 = rng.choice([3, 5, 8, 14]), rng.choice([3, 6, 14])
    if wide == "big":  # a pool of 65..200 bases (big keys)
        v0, v1 = rng.choice([(65, 6), (8, 100), (100, 110), (70, 40), (200, 20)])
    elif wide:        # a pool of 33..64 bases (wide keys), the other short or long
        v0, v1 = rng.choice([(33, 6), (8, 40), (64, 64), (36, 33)])
    alphabet = rng.choice(["AC", BASES, BASES])
    p0 = make_pool(rng, rng.choice([1, 4, 30]), v0, alphabet, iupac_rate=rng.choice([0, 0, 0.05 if v0 <= 64 else 0.01]))
    p1 = make_pool(rng, rng.choice([1, 4, 30]), v1, alphabet, iupac_rate=rng.choice([0, 0, 0.05 if v1 <= 64 else 0.01]))
    template = make_template(rng, 2, [v0, v1], rng.choice([0, 1, 3]), rng.choice([4, 8, 12]))
    strand = rng.choice([0, 1, 2])
    mm = rng.choice([0, 1, 2, 3])
    first = rng.random() < 0.5
    reads = make_reads(rng, template, [p0, p1], rng.choice(sizes), strand, rng.choice([0, 0.03, 0.08]), rng.choice([0, 0.02]),
                       rng.choice([0, 0.3]), 0.1, rng.choice([0, 5, 30]))
    return dict(kind="combo", template=template, strand=strand, pool0=p0, pool1=p1, mismatches=mm, use_first=first, reads=reads)


def random_dual_case(rng: random.Random, hazard_free: bool = True, sizes=(1, 30, 150), max_mm: int = 2, wide: bool = False) -> dict:
    l1, l2 = rng.choice([4, 6, 9, 12]), rng.choice([4, 7, 12])
    if wide == "big":  # a barcode of 65..240 bases on either mate (big keys for both)
        l1, l2 = rng.choice([(65, 7), (9, 100), (128, 129), (70, 34), (240, 240)])
    elif wide:        # a barcode of 33..64 bases on either mate (wide keys for both)
        l1, l2 = rng.choice([(33, 7), (9, 40), (64, 64), (35, 34)])
    mm1, mm2 = rng.randint(0, max_mm), rng.randint(0, max_mm)
    # pools whose members are >= 2*cap+1 apart cannot trigger the reference's order-dependent
    # segmented-search cache
    d1 = 2 * mm1 + 1 if hazard_free else 1
    d2 = 2 * mm2 + 1 if hazard_free else 1
    u1 = make_pool(rng, rng.choice([1, 3, 8]), l1, BASES, min_dist=d1)
    u2 = make_pool(rng, rng.choice([1, 3, 8]), l2, BASES, min_dist=d2)
    allpairs = [(a, b) for a in u1 for b in u2]
    rng.shuffle(allpairs)
    pairs = allpairs[: rng.randint(1, len(allpairs))]
    pool1 = [a for a, _ in pairs]
    pool2 = [b for _, b in pairs]
    t1 = make_template(rng, 1, [l1], rng.choice([0, 2, 4]), rng.choice([4, 8]))
    t2 = make_template(rng, 1, [l2], rng.choice([0, 2, 4]), rng.choice([4, 8]))
    rev1, rev2 = rng.random() < 0.3, rng.random() < 0.3
    randomized = rng.random() < 0.4
    first = rng.random() < 0.5
    n = rng.choice(sizes)
    r1s, r2s = [], []
    p_sub, p_n = rng.choice([0, 0.03, 0.08]), rng.choice([0, 0.02])
    for _ in range(n):
        u = rng.random()
        if u < 0.1:
            a, b = rand_seq(rng, rng.randint(0, 30)), rand_seq(rng, rng.randint(0, 30))
        else:
            if u < 0.8:
                x, y = rng.choice(pairs)
            else:
                x, y = rng.choice(u1), rng.choice(u2)
            a = mutate(rng, fill_template(t1, [x]), p_sub, p_n, 0.05)
            b = mutate(rng, fill_template(t2, [y]), p_sub, p_n, 0.05)
            pad = rng.choice([0, 4, 20])
            a = rand_seq(rng, rng.randint(0, pad)) + a + rand_seq(rng, rng.randint(0, pad))
            b = rand_seq(rng, rng.randint(0, pad)) + b + rand_seq(rng, rng.randint(0, pad))
            if rng.random() < 0.1:
                x2, _ = rng.choice(pairs)
                a += mutate(rng, fill_template(t1, [x2]), p_sub, p_n, 0.0)
            if rev1:
                a = rc(a)
            if rev2:
                b = rc(b)
            if randomized and rng.random() < 0.5:
                a, b = b, a
        r1s.append(a)
        r2s.append(b)
    return dict(kind="dual", template1=t1, reverse1=rev1, mismatches1=mm1, pool1=pool1,
                template2=t2, reverse2=rev2, mismatches2=mm2, pool2=pool2,
                randomized=randomized, use_first=first, reads1=r1s, reads2=r2s)


def random_paired_combo_case(rng: random.Random, sizes=(1, 30, 150), max_mm: int = 2, wide: bool = False) -> dict:
    """countPairedComboBarcodes: the reads of a dual case against the two pools taken independently
    (distinct barcodes, no list of valid pairs; close barcodes allowed so that ties occur)."""
    c = random_dual_case(rng, hazard_free=rng.random() < 0.5, sizes=sizes, max_mm=max_mm, wide=wide)
    pool1 = list(dict.fromkeys(c["pool1"]))
    pool2 = list(dict.fromkeys(c["pool2"]))
    return dict(kind="paired_combo", template1=c["template1"], reverse1=c["reverse1"], mismatches1=c["mismatches1"], pool1=pool1,
                template2=c["template2"], reverse2=c["reverse2"], mismatches2=c["mismatches2"], pool2=pool2,
                randomized=c["randomized"], use_first=c["use_first"], reads1=c["reads1"], reads2=c["reads2"])


def random_dual_single_end_case(rng: random.Random, sizes=(1, 30, 150), wide: bool = None, diag: bool = False, nreg: int = None) -> dict:
    """countDualBarcodesSingleEnd: the variable regions of one read, pools aligned by row (row c = valid combination c);
    `wide` forces a combined key longer than 32 bases; nreg >= 3 exercises templates with many regions."""
    if nreg is None:
        nreg = 2 if diag else rng.choice([1, 2, 2])
    if wide is None:
        wide = rng.random() < 0.4
    if wide == "big":      # a combined key of 65..256 bases
        lens = rng.choice({1: [[65], [100], [230]], 2: [[40, 40], [20, 100], [100, 100], [70, 5]], 3: [[40, 40, 40], [30, 5, 90]], 4: [[20, 30, 40, 50]],
                           5: [[30, 30, 30, 30, 30]]}[nreg])
    elif nreg >= 3:
        lens = rng.choice({3: [[4, 6, 5], [8, 8, 8], [12, 20, 10], [20, 20, 20], [3, 30, 7]], 4: [[4, 4, 4, 4], [10, 10, 10, 10], [16, 16, 16, 16]],
                           5: [[3, 4, 5, 6, 7], [12, 12, 12, 12, 12]]}[nreg])
    elif nreg == 1:
        lens = [rng.choice([33, 40, 64] if wide else [4, 9, 20])]
    else:
        # (include.invalid=TRUE searches each region on its own with the narrow index: regions <= 32 bases there)
        lens = rng.choice(([[20, 20], [17, 30], [32, 32]] if diag else [[20, 20], [17, 30], [32, 32], [5, 40]]) if wide else [[4, 6], [8, 8], [12, 20]])
    alphabet = rng.choice(["AC", BASES])
    n = min(rng.choice([1, 4, 25]), len(alphabet) ** min(sum(lens), 8) // 2)      # distinct rows must exist
    seen, rows = set(), []
    while len(rows) < n:
        row = tuple(rand_seq(rng, l, alphabet) for l in lens)
        if diag and rows and rng.random() < 0.4:      # a barcode shared by several combinations (duplicates within one column)
            row = (rng.choice(rows)[0], row[1]) if rng.random() < 0.5 else (row[0], rng.choice(rows)[1])
        if "".join(row) not in seen:
            seen.add("".join(row))
            rows.append(row)
    pools = [[row[r] for row in rows] for r in range(nreg)]
    template = make_template(rng, nreg, lens, rng.choice([0, 2, 5]), rng.choice([5, 9]))
    strand = rng.choice([0, 1, 2])
    mm = rng.randint(0, 3)
    first = rng.random() < 0.5
    reads = []
    p_sub, p_n = rng.choice([0, 0.01, 0.04]), rng.choice([0, 0.01])
    for _ in range(rng.choice(sizes)):
        u = rng.random()
        if u < 0.1:
            reads.append(rand_seq(rng, rng.randint(0, len(template) + 20)))
            continue
        row = rng.choice(rows) if u < 0.85 else tuple(rng.choice(rows)[r] for r in range(nreg))   # some mixed (invalid) rows
        core = mutate(rng, fill_template(template, list(row)), p_sub, p_n, 0.05)
        read = rand_seq(rng, rng.randint(0, 12)) + core + rand_seq(rng, rng.randint(0, 12))
        if strand == 1 or (strand == 2 and rng.random() < 0.5):
            read = rc(read)
        reads.append(read)
    return dict(kind="dual_single_end", template=template, strand=strand, pools=pools, mismatches=mm, use_first=first, reads=reads)


def random_big_match_case(rng: random.Random) -> dict:
    """matchBarcodes with choices of 65..256 bases (big keys)."""
    vlen = rng.choice([65, 100, 128, 200, 256])
    pool = make_pool(rng, rng.choice([1, 5, 30]), vlen, "ACGT")
    seqs = [mutate(rng, rng.choice(pool), 0.01, 0.003, 0.1) for _ in range(30)]
    subs, rev = rng.choice([0, 1, 2, 3]), rng.random() < 0.5
    if rev:
        seqs = [rc(s) if set(s.upper()) <= set("ACGT") else s for s in seqs]
    return dict(kind="match", sequences=seqs, choices=pool, substitutions=subs, reverse=rev)


def large_grid_case(seed: int = 77, n_pool: int = 40000, n_reads: int = 21000) -> dict:
    """countComboBarcodes with 2 x 40 000 barcodes (1.6e9 possible combinations: beyond any dense histogram), the inputs
    regenerated from a seed wherever they are needed (tests/golden/kaori_large_grid.json holds a digest of them)."""
    rng = random.Random(seed)

    def pool(length):
        seen = set()
        while len(seen) < n_pool:
            seen.add(rand_seq(rng, length))
        out = sorted(seen)
        rng.shuffle(out)
        return out
    pool0, pool1 = pool(12), pool(10)
    template = "ACGT" + "-" * 12 + "GGTACC" + "-" * 10 + "TTGA"
    pairs = [(rng.randrange(n_pool), rng.randrange(n_pool)) for _ in range(3000)]
    reads = []
    for _ in range(n_reads):
        a, b = rng.choice(pairs) if rng.random() < 0.7 else (rng.randrange(n_pool), rng.randrange(n_pool))
        s = fill_template(template, [pool0[a], pool1[b]])
        s = rand_seq(rng, rng.randrange(0, 20)) + s + rand_seq(rng, rng.randrange(0, 20))
        if rng.random() < 0.3:
            s = rc(s)
        reads.append(mutate(rng, s, 0.01, 0.002, 0.0))
    return dict(kind="combo", template=template, strand=2, pool0=pool0, pool1=pool1, mismatches=1, use_first=True, reads=reads)


def case_digest(case: dict) -> str:
    import hashlib
    h = hashlib.sha256()
    for key in sorted(case):
        v = case[key]
        h.update(key.encode())
        h.update(("\n".join(v) if isinstance(v, list) else repr(v)).encode())
    return h.hexdigest()


def random_random_barcode_case(rng: random.Random, sizes=(1, 30, 150)) -> dict:
    """countRandomBarcodes: unknown sequences in the variable region; asymmetric flanks exercise the
    reference's use of forward coordinates on the reverse strand, lower case / N its string handling."""
    vlen = rng.choice([3, 6, 10, 20, 40])
    template = make_template(rng, 1, [vlen], rng.choice([0, 2, 5]), rng.choice([5, 9, 14]))
    strand = rng.choice([0, 1, 2])
    mm = rng.randint(0, 2)
    first = rng.random() < 0.5
    alphabet = rng.choice(["AC", BASES])
    some = [rand_seq(rng, vlen, alphabet) for _ in range(rng.choice([1, 3, 10]))]
    reads = []
    p_sub, p_n, p_low = rng.choice([0, 0.02, 0.06]), rng.choice([0, 0.02]), rng.choice([0, 0.1])
    for _ in range(rng.choice(sizes)):
        if rng.random() < 0.1:
            reads.append(rand_seq(rng, rng.randint(0, len(template) + 20)))
            continue
        core = mutate(rng, fill_template(template, [rng.choice(some)]), p_sub, p_n, p_low)
        read = rand_seq(rng, rng.randint(0, 12)) + core + rand_seq(rng, rng.randint(0, 12))
        if rng.random() < 0.15:
            read += rand_seq(rng, rng.randint(0, 3)) + mutate(rng, fill_template(template, [rng.choice(some)]), p_sub, p_n, p_low)
        if strand == 1 or (strand == 2 and rng.random() < 0.5):
            read = rc(read)
        reads.append(read)
    return dict(kind="random", template=template, strand=strand, mismatches=mm, use_first=first, reads=reads)


def random_match_case(rng: random.Random) -> dict:
    vlen = rng.choice([3, 5, 8, 12])
    alphabet = rng.choice(["AC", BASES])
    pool = make_pool(rng, rng.choice([1, 4, 30]), vlen, alphabet, iupac_rate=rng.choice([0, 0.1]))
    seqs = [mutate(rng, concrete(rng, rng.choice(pool)), 0.15, 0.03, 0.1) for _ in range(40)]
    return dict(kind="match", sequences=seqs, choices=pool, substitutions=rng.choice([0, 1, 2, 3]), reverse=rng.random() < 0.5)


def write_bgzf(path: str, data: bytes, block: int = 60000, level: int = 6, eof_block: bool = True) -> None:
    """BGZF ("blocked gzip", SAM/BAM specification section 4.1; what bgzip writes): a series of gzip members of at most
    64 KiB, each carrying its own compressed size in a 'BC' extra subfield, optionally ended by the empty EOF member."""
    import struct
    import zlib

    def member(chunk: bytes) -> bytes:
        co = zlib.compressobj(level, zlib.DEFLATED, -15)
        body = co.compress(chunk) + co.flush()
        bsize = 12 + 6 + len(body) + 8
        assert bsize <= 65536
        head = b"\x1f\x8b\x08\x04" + b"\x00\x00\x00\x00" + b"\x00\xff" + struct.pack("<H", 6) + b"BC" + struct.pack("<HH", 2, bsize - 1)
        return head + body + struct.pack("<II", zlib.crc32(chunk) & 0xFFFFFFFF, len(chunk) & 0xFFFFFFFF)

    with open(path, "wb") as f:
        for a in range(0, len(data), block):
            f.write(member(data[a:a + block]))
        if eof_block:
            f.write(member(b""))


def fastq_text(reads, name_prefix: str = "r", trailing_newline: bool = True) -> bytes:
    out = b"".join(b"@%s%d some comment\n" % (name_prefix.encode(), i) + (r.encode() if isinstance(r, str) else bytes(r)) + b"\n+\n" +
                   b"I" * len(r) + b"\n" for i, r in enumerate(reads))
    return out if trailing_newline else out[:-1]


def fastq_record(i: int, read, flaw: str = None, name_prefix: str = "r", rng: random.Random = None) -> bytes:
    """One FASTQ record as `fastq_text` writes it, or one of the forms only the sequential reader accepts or reports:

    * "multiline": sequence and quality each split over two lines (legal, FastqReader.hpp:66-84);
    * "oversized": the read padded with random bases to ~16 KB, longer than the parallel reader's window under a small
      $SCG_FASTQ_PIECE_KB (legal);
    * "malformed": a quality string one byte shorter than the sequence (illegal: the reference's error)."""
    s = read.encode() if isinstance(read, str) else bytes(read)
    head = b"@%s%d some comment\n" % (name_prefix.encode(), i)
    if flaw is None:
        return head + s + b"\n+\n" + b"I" * len(s) + b"\n"
    if flaw == "multiline":
        if len(s) < 2:
            raise ValueError("a multi-line record needs a read of at least 2 bases")
        h = len(s) // 2
        return head + s[:h] + b"\n" + s[h:] + b"\n+\n" + b"I" * h + b"\n" + b"I" * (len(s) - h) + b"\n"
    if flaw == "oversized":
        s += rand_seq(rng or random.Random(i), 16 * 1024).encode()
        return head + s + b"\n+\n" + b"I" * len(s) + b"\n"
    if flaw == "malformed":
        s = s or b"A"
        return head + s + b"\n+\n" + b"I" * (len(s) - 1) + b"\n"
    raise ValueError(f"unknown flaw {flaw!r}")


def write_flawed_fastq(path, reads, flaws: dict = None, seed: int = 0) -> str:
    """A FASTQ file of strict 4-line records except at the record indices of `flaws` ({index: kind}, kinds as in
    `fastq_record`).  For a paired run, call it once per mate with each mate's own flaws.  The expected result is always
    taken from parsing the written file with the oracle, never from `reads` (a multi-line or oversized record changes
    neither the read nor the count of reads, but a flaw the reference rejects ends the parse)."""
    rng = random.Random(seed)
    flaws = flaws or {}
    with open(path, "wb") as f:
        for i, r in enumerate(reads):
            f.write(fastq_record(i, r, flaws.get(i), rng=rng))
    return str(path)


# ---------------------------------------------------------------------------------------------
# Constructed inputs for the staged kernels' tile and dispatch boundaries (tests/test_gpu_tile_edges.py).
# ---------------------------------------------------------------------------------------------
def segments_template(rng: random.Random, segments) -> str:
    """[("c", n) | ("v", n), ...] -> template: n random constant bases or n '-' per segment."""
    return "".join(rand_seq(rng, n) if kind == "c" else "-" * n for kind, n in segments)


def seed_blocks(positions, max_mm: int, seed_max: int = 9, max_seeds: int = 4) -> list[int]:
    """Blocks (of 32 template positions) of the pigeonhole seeds the host chooses for the constant positions of one strand
    (mirror of build_scan in scg_library.cpp): runs of up to seed_max consecutive constant positions inside one block,
    the longest first, earlier ones first among equals; runs are split when there are fewer than max_mm + 1."""
    want = max_mm + 1
    if want > max_seeds or len(positions) < want:
        return []
    runs = []
    k = 0
    while k < len(positions):
        blk = positions[k] >> 5
        n = 1
        while k + n < len(positions) and n < seed_max and positions[k + n] >> 5 == blk:
            n += 1
        runs.append([k, n, blk])
        k += n
    while len(runs) < want:
        big = max(range(len(runs)), key=lambda i: (runs[i][1], -i))
        first, n, blk = runs[big]
        if n < 2:
            break
        runs[big:big + 1] = [[first, n // 2, blk], [first + n // 2, n - n // 2, blk]]
    if len(runs) < want:
        return []
    chosen = sorted(runs, key=lambda r: -r[1])[:want]       # stable: earlier runs first among equals
    return [r[2] for r in chosen]


def compact_ok(template: str, max_mm: int) -> bool:
    """Whether the host allows the compact candidate form (NC = 3) for this template: every seed of both strands lies in
    template block 0 or 1."""
    L = len(template)
    fpos = [i for i, c in enumerate(template) if c != "-"]
    rpos = sorted(L - 1 - i for i in fpos)
    return all(b <= 1 for b in seed_blocks(fpos, max_mm) + seed_blocks(rpos, max_mm))


def chance_hits(template: str, max_mm: int, read_len: int) -> float:
    """expected_chance_hits of scg_kernels.hip: windows of a random read that pass the template's constant bases."""
    c = sum(ch != "-" for ch in template)
    ways, choose, pow3 = 0.0, 1.0, 1.0
    for k in range(min(max_mm, c) + 1):
        ways += choose * pow3
        choose = choose * (c - k) / (k + 1)
        pow3 *= 3
    return (read_len - len(template) + 1 if read_len > len(template) else 1) * ways / 4.0 ** c


class Filler:
    """Fast random ACGT padding: slices of one long random string."""

    def __init__(self, seed: int, size: int = 1 << 16):
        self.rng = random.Random(seed)
        self.text = rand_seq(self.rng, size)

    def __call__(self, n: int) -> str:
        if n <= 0:
            return ""
        a = self.rng.randrange(0, len(self.text) - n)
        return self.text[a:a + n]


def place(fill: Filler, construct: str, n: int, pos: int) -> str:
    """A read of n bases holding `construct` at position pos, random bases around it."""
    assert 0 <= pos and pos + len(construct) <= n, (pos, len(construct), n)
    return fill(pos) + construct + fill(n - pos - len(construct))


def substitute(s: str, i: int, c: str = None) -> str:
    """s with base i replaced by c (default: a different base)."""
    if c is None:
        c = "A" if s[i].upper() != "A" else "C"
    return s[:i] + c + s[i + 1:]


def split_pair(fill: Filler, construct: str, k: int, n1: int, n2: int) -> tuple[str, str]:
    """Two neighbouring reads: the first (n1 bases) ends with the construct's first k bases, the second (n2 bases)
    starts with the rest."""
    return fill(n1 - k) + construct[:k], construct[k:] + fill(n2 - (len(construct) - k))


# ---------------------------------------------------------------------------------------------
# Crowded pools: "star and ladder" libraries whose entries sit one or two substitutions apart, at the positions where the
# index's position groups begin and end, and queries built for a known outcome (tests/test_crowded_cpu.py checks the
# outcomes with a brute force; tests/test_gpu_crowded.py runs them through every matcher path).
# ---------------------------------------------------------------------------------------------
IUPAC_SETS = {"A": "A", "C": "C", "G": "G", "T": "T", "R": "AG", "Y": "CT", "S": "CG", "W": "AT", "K": "GT", "M": "AC",
              "B": "CGT", "D": "AGT", "H": "ACT", "V": "ACG", "N": "ACGT"}
_ONE_HOT = {"A": 1, "C": 2, "G": 4, "T": 8}
_SET_BITS = {c: sum(_ONE_HOT[b] for b in s) for c, s in IUPAC_SETS.items()}
CROWDED_SHORT = 16      # below this length a pool stays inside {A, C, G}: see crowded_pool


def crowded_positions(length: int) -> list[int]:
    """Both ends, both sides of every half and quarter slice edge of the index builders (floor(k * length / parts)), and both
    sides of the 32-, 64-, 128- and 192-bit word edges of the key planes."""
    want = {0, length - 1, 31, 32, 63, 64, 127, 128, 191, 192}
    for parts in (2, 4):
        for k in range(parts + 1):
            want.update((k * length // parts - 1, k * length // parts))
    return sorted(p for p in want if 0 <= p < length)


def position_groups(length: int, budget: int) -> list[frozenset]:
    """The position groups of an index built for `budget` (finish_index, finish_index_n): the whole key, its halves, the six
    pairs of quarters, the quarters; none for wider budgets (dense scans)."""
    def part(i, parts):
        return frozenset(range(i * length // parts, (i + 1) * length // parts))
    if budget == 0:
        return [part(0, 1)]
    if budget == 1:
        return [part(0, 2), part(1, 2)]
    if budget == 2:
        return [part(a, 4) | part(b, 4) for a, b in ((0, 1), (2, 3), (0, 2), (1, 3), (0, 3), (1, 2))]
    if budget == 3:
        return [part(q, 4) for q in range(4)]
    return []


def _quarter(length: int, p: int) -> int:
    return next(q for q in range(4) if q * length // 4 <= p < (q + 1) * length // 4)


def _bits(s: str, table: dict) -> int:
    """4 bits per position: the bases a library string allows (_SET_BITS), or the one base a query holds (_ONE_HOT; none for
    any other byte).  The Hamming distance is then length - popcount(entry & query)."""
    v = 0
    for i, c in enumerate(s.upper()):
        v |= table.get(c, 0) << (4 * i)
    return v


def crowded_outcome(pool_bits: list[int], query: str, cap: int):
    """("hit", distance, index) for a unique minimum within cap, ("tie", distance, indices), or ("miss", minimum, None)."""
    q = _bits(query, _ONE_HOT)
    dist = [len(query) - (e & q).bit_count() for e in pool_bits]
    best = min(dist)
    if best > cap:
        return "miss", best, None
    who = [i for i, d in enumerate(dist) if d == best]
    return ("hit", best, who[0]) if len(who) == 1 else ("tie", best, who)


class CrowdedPool(list):
    """The library strings, with what they were built from: `stars` = [(centre, {position: substituted base}, {position:
    bases that some entry of the star allows there})], one per centre; `positions` = crowded_positions(length); `alphabet`
    of the centres."""
    stars: list
    positions: list
    alphabet: str


def crowded_pool(rng: random.Random, length: int, budget: int, centres: int = 6, arms: int = None, doubles: int = 3,
                 iupac: bool = None, alphabet: str = None, min_dist: int = None) -> CrowdedPool:
    """A library of `centres` stars: per centre, the centre with one base substituted at p for (up to `arms` of) the positions
    p of crowded_positions, `doubles` entries with two of those substitutions in different quarter slices (more for a wider
    budget), and -- in about half the pools -- the centre itself.  In keys of up to 64 bases, two of a star's one-substitution
    entries carry a two-base IUPAC code at p instead (the substituted base and another one, not the centre's), so that no two
    entries share an expansion.

    Below CROWDED_SHORT bases the pool stays inside {A, C, G}^length: in so small a space every query would otherwise lie
    within a wide cap of some entry, and neither a miss beyond the cap nor a unique hit at a distance could be built; a
    query's T then mismatches every entry.  `alphabet` and `min_dist` (between the centres) override that."""
    if alphabet is None:
        alphabet = "ACG" if length < CROWDED_SHORT else BASES
    P = crowded_positions(length)
    use = P if arms is None else sorted(rng.sample(P, min(arms, len(P))))
    if iupac is None:
        iupac = length <= 64
    cs = make_pool(rng, centres, length, alphabet, min_dist=min(3, length) if min_dist is None else min_dist)
    assert len(cs) == centres
    keep_centre = rng.random() < 0.5
    seen, out, stars = set(), CrowdedPool(), []

    def add(s):
        exp = [s]
        for i, c in enumerate(s):
            if c not in BASES:
                exp = [e[:i] + b + e[i + 1:] for e in exp for b in IUPAC_SETS[c]]
        if not seen.intersection(exp):
            seen.update(exp)
            out.append(s)

    for c in cs:
        alt = {p: rng.choice([b for b in alphabet if b != c[p]]) for p in use}
        avoid = {p: c[p] + alt[p] for p in use}
        arm = dict(alt)
        if iupac:
            for p in rng.sample(use, min(2, len(use))):
                other = rng.choice([b for b in alphabet if b not in avoid[p]])
                avoid[p] += other
                arm[p] = next(k for k, v in IUPAC_SETS.items() if set(v) == {alt[p], other})
        stars.append((c, alt, avoid))
        if keep_centre:
            add(c)
        for p in use:
            add(substitute(c, p, arm[p]))
        made = 0
        for _ in range(50):
            if made >= doubles + max(budget - 2, 0) or len(use) < 2:
                break
            p, r = rng.sample(use, 2)
            if _quarter(length, p) != _quarter(length, r):
                add(substitute(substitute(c, p, alt[p]), r, alt[r]))
                made += 1
    order = list(out)
    rng.shuffle(order)
    out[:] = order
    out.stars, out.positions, out.alphabet = stars, P, alphabet
    return out


def _third(rng, pool: CrowdedPool, star: int, p: int) -> str:
    """a base at p that no entry of the star allows there; one outside the pool's alphabet where there is one"""
    c, _, avoid = pool.stars[star]
    free = [b for b in BASES if b not in avoid.get(p, c[p])]
    return rng.choice([b for b in free if b not in pool.alphabet] or free)


def _spread(rng, length: int, P: list, n: int, turn: int, fixed=()) -> list:
    """n positions of P outside `fixed`, in as many different quarter slices as possible; `turn` rotates through the choices
    of quarters so that every position group is in turn the only one left intact."""
    import itertools
    by_q = [[p for p in P if _quarter(length, p) == q and p not in fixed] for q in range(4)]
    free = [q for q in range(4) if by_q[q] and q not in {_quarter(length, f) for f in fixed}]
    picks = []
    k = min(n, len(free))
    if k:
        combos = list(itertools.combinations(free, k))
        for q in combos[turn % len(combos)]:
            picks.append(rng.choice(by_q[q]))
    rest = [p for p in P if p not in picks and p not in fixed]
    rng.shuffle(rest)
    picks += rest[:n - len(picks)]
    if len(picks) < n:
        others = [p for p in range(length) if p not in picks and p not in fixed and p not in P]
        picks += rng.sample(others, n - len(picks))
    return picks


def crowded_query(rng, pool: CrowdedPool, kind: str, d: int, turn: int = 0, star: int = None):
    """One query of the wanted kind against one star of the pool, or None where the key is too short for it:
    "hit": a one-substitution entry with d further bases changed to third bases (distance d from it, d + 1 or more from the
    rest of the star); "tie": the centre with the substitutions of two entries p and r and d - 1 third bases (distance d from
    both); "centre": the centre with d third bases."""
    length = len(pool[0])
    star = rng.randrange(len(pool.stars)) if star is None else star
    c, alt, _ = pool.stars[star]
    arms = sorted(alt)
    q = list(c)
    if kind == "tie":
        if len(arms) < 2 or d < 1 or d + 1 > length:
            return None
        by_q = {}
        for p in arms:
            by_q.setdefault(_quarter(length, p), []).append(p)
        qs = sorted(by_q)
        if len(qs) >= 2:
            qa, qb = [(a, b) for a in qs for b in qs if a != b][turn % (len(qs) * (len(qs) - 1))]
            p, r = rng.choice(by_q[qa]), rng.choice(by_q[qb])
        else:
            p, r = rng.sample(arms, 2)
        q[p], q[r] = alt[p], alt[r]
        for s in _spread(rng, length, pool.positions, d - 1, turn // 12, fixed=(p, r)):
            q[s] = _third(rng, pool, star, s)
    else:
        fixed = ()
        if kind == "hit":
            mine = [p for p in arms if _quarter(length, p) == turn % 4] or arms
            p = rng.choice(mine)
            q[p] = alt[p]
            fixed = (p,)
        if d + len(fixed) > length:
            return None
        for s in _spread(rng, length, pool.positions, d, turn // 4, fixed=fixed):
            q[s] = _third(rng, pool, star, s)
    return "".join(q)


def crowded_queries(rng: random.Random, pool: CrowdedPool, budget: int, n: int = 240, annotate: bool = False) -> list:
    """n queries for a cap of `budget`, each built for its outcome and kept only if a Hamming count confirms it: 36 % ties
    between two entries at each distance 1..budget, 36 % unique hits at each distance 1..budget, 16 % misses one substitution
    beyond the cap, the rest exact hits; the mismatches sit on crowded_positions and rotate through the quarter slices.  One
    query in eight then gets a byte that is no base at a random or a crowded position (whatever that makes of it), one in
    six lower case.  annotate=True: (query, kind, distance) instead of the query."""
    bits = [_bits(s, _SET_BITS) for s in pool]
    out = []

    def fill(kind, want_kind, d, count):
        got, turn = 0, rng.randrange(12)
        for attempt in range(40 * count + 40):
            if got >= count:
                break
            q = crowded_query(rng, pool, kind, d, turn + attempt)
            if q is None:
                continue
            k, dist, _ = crowded_outcome(bits, q, budget)
            ok = (k == "miss" and dist == budget + 1) if want_kind == "miss" else (k == want_kind and dist == d)
            if ok:
                out.append((q, want_kind, d))
                got += 1

    for d in range(1, budget + 1):
        fill("tie", "tie", d, (36 * n) // (100 * budget))
        fill("hit", "hit", d, (36 * n) // (100 * budget))
    fill("hit", "miss", budget + 1, (16 * n) // 100)
    exact = [s for s in pool if set(s) <= set(BASES)]
    while len(out) < n:
        out.append((rng.choice(exact), "hit", 0))
    rng.shuffle(out)
    P = pool.positions
    for i, (q, kind, d) in enumerate(out):
        if i % 8 == 3:
            at = rng.choice(P) if i % 16 == 3 else rng.randrange(len(q))
            q = q[:at] + rng.choice("NnX.") + q[at + 1:]
            k, dist, _ = crowded_outcome(bits, q, budget)
            kind, d = k, dist
        if i % 6 == 1:
            q = q.lower() if i % 12 == 1 else "".join(ch.lower() if rng.random() < 0.5 else ch for ch in q)
        out[i] = (q, kind, d)
    return out if annotate else [q for q, _, _ in out]


def _embed(rng, template: str, inserts: list, c: int, pad: int) -> str:
    """The construct with c substitutions in its constant bases, random bases around it."""
    core = list(fill_template(template, inserts))
    const = [i for i, ch in enumerate(template) if ch != "-"]
    for p in rng.sample(const, c):
        core[p] = rng.choice([b for b in BASES if b != core[p]])
    return rand_seq(rng, rng.randint(0, pad)) + "".join(core) + rand_seq(rng, rng.randint(0, pad))


def crowded_match_case(seed: int, length: int, budget: int, reverse: bool, n: int = 200) -> dict:
    """matchBarcodes over a crowded pool; reverse=True hands the same queries over reverse-complemented."""
    rng = random.Random(f"match {seed} {length} {budget}")
    pool = crowded_pool(rng, length, budget)
    seqs = crowded_queries(rng, pool, budget, n)
    if reverse:
        seqs = [rc(s) for s in seqs]
    return dict(kind="match", sequences=seqs, choices=list(pool), substitutions=budget, reverse=reverse)


def crowded_single_case(seed: int, length: int, budget: int, use_first: bool, n_reads: int = 2000) -> dict:
    """countSingleBarcodes, both strands, flanks of 10 constant bases: a read with c = 0..budget substitutions in the flanks
    carries a query built for the remaining cap of budget - c (a few carry one substitution too many); where two constructs
    fit into a read (80 bases, 150 for keys beyond 64), one read in ten holds a second one right behind the first."""
    rng = random.Random(f"single {seed} {length} {budget}")
    pool = crowded_pool(rng, length, budget)
    template = rand_seq(rng, 10) + "-" * length + rand_seq(rng, 10)
    per_cap = [crowded_queries(rng, pool, cap, 120) for cap in range(budget + 1)]
    longest = 150 if length > 64 else 80
    pad = min(10, longest - len(template)) // 2

    def construct():
        c = rng.choice(list(range(budget + 1)) * 3 + [budget + 1])
        q = rng.choice(per_cap[max(budget - c, 0)])
        return _embed(rng, template, [q], c, 0)

    reads = []
    for _ in range(n_reads):
        one = construct()
        if rng.random() < 0.1 and 2 * len(template) <= longest:
            read = one + construct()
        else:
            read = rand_seq(rng, rng.randint(0, pad)) + one + rand_seq(rng, rng.randint(0, pad))
        reads.append(rc(read) if rng.random() < 0.5 else read)
    return dict(kind="single", template=template, strand=2, pool=list(pool), mismatches=budget, use_first=use_first, reads=reads)


def crowded_combo_case(seed: int, lens: tuple, budget: int, use_first: bool = True, n_reads: int = 2000) -> dict:
    """countComboBarcodes, both pools crowded, both strands.  The two regions share one budget, spent in order (SURVEY.md
    A.5): the first region's query lies at a known distance d0 from its entry -- 0, 1, all of the budget, or anything
    between -- and the second region's query is built for the cap of budget - d0 - c that is left."""
    rng = random.Random(f"combo {seed} {lens} {budget}")
    p0, p1 = crowded_pool(rng, lens[0], budget), crowded_pool(rng, lens[1], budget)
    template = rand_seq(rng, 8) + "-" * lens[0] + rand_seq(rng, 6) + "-" * lens[1] + rand_seq(rng, 8)
    first = crowded_queries(rng, p0, budget, 240, annotate=True)
    by_d = {}
    for q, kind, d in first:
        by_d.setdefault(d if kind == "hit" else -1, []).append(q)         # -1: ties and misses
    rest = [crowded_queries(rng, p1, cap, 120) for cap in range(budget + 1)]
    reads = []
    for _ in range(n_reads):
        d0 = rng.choice([0, 1, budget, budget, -1] + list(range(budget + 1)))
        d0 = d0 if d0 in by_d else 0
        c = rng.choice([0, 0, 0, 1]) if d0 >= 0 and d0 < budget else 0
        q0 = rng.choice(by_d[d0])
        q1 = rng.choice(rest[max(budget - max(d0, 0) - c, 0)])
        read = _embed(rng, template, [q0, q1], c, 6)
        if rng.random() < 0.08:
            read += _embed(rng, template, [rng.choice(by_d[0]), rng.choice(rest[budget])], 0, 0)
        reads.append(rc(read) if rng.random() < 0.5 else read)
    return dict(kind="combo", template=template, strand=2, pool0=list(p0), pool1=list(p1), mismatches=budget, use_first=use_first, reads=reads)


def crowded_dual_case(seed: int, lens: tuple, budgets: tuple, randomized: bool, use_first: bool, n_reads: int = 1500) -> dict:
    """countDualBarcodes (and its diagnostics form, and countPairedComboBarcodes over the distinct barcodes).  Mate 1's
    barcodes form a crowded pool: near a centre, five or more of them lie within the cap, more than pair_match gathers
    before it falls back to the nested search.  Mate 2's form stars of three entries, centres far apart: never more than
    four within the cap.  The valid pairs are a strict subset of the cross product in which barcodes recur (several rows
    per barcode): every mate-1 barcode has one or two partners, and two arms p, r of each mate-1 star share a partner, a
    third arm of the star has another.  Read pairs: the centre of a mate-1 star, all its arms within the cap; a tie between the two arms over their shared partner (two valid pairs
    at the same total), the same tie over the other arm's partner (only invalid pairs within the caps) or with one arm
    nearer (a unique best pair), a valid row with each mate near its barcode, or two unrelated queries.
    case["probes"] holds the (query 1, query 2) of every pair as built, before flanks, padding and strands."""
    rng = random.Random(f"dual {seed} {lens} {budgets}")
    l1, l2 = lens
    m1, m2 = budgets
    u1 = crowded_pool(rng, l1, m1, iupac=False)
    if l2 < CROWDED_SHORT:       # short keys: four centres that differ nearly everywhere, over all four bases
        u2 = crowded_pool(rng, l2, m2, centres=4, arms=2, doubles=0, iupac=False, alphabet=BASES, min_dist=l2 - 1)
    else:
        u2 = crowded_pool(rng, l2, m2, centres=5, arms=2, doubles=0, iupac=False)
    s1, s2 = set(u1), list(u2)
    rows, special = [], []
    for c, alt, _ in u1.stars:
        arms = [p for p in sorted(alt) if substitute(c, p, alt[p]) in s1]
        rng.shuffle(arms)
        if len(arms) >= 3:
            p, r, t = arms[:3]
            x, y = rng.sample(s2, 2)
            rows += [(substitute(c, p, alt[p]), x), (substitute(c, r, alt[r]), x), (substitute(c, t, alt[t]), y)]
            special.append((len(special), p, r, t, x, y))
    taken = {a for a, _ in rows}
    for a in u1:
        if a not in taken:
            rows += [(a, b) for b in rng.sample(s2, rng.choice([1, 1, 2]))]
    rng.shuffle(rows)
    t1 = rand_seq(rng, 6) + "-" * l1 + rand_seq(rng, 6)
    t2 = rand_seq(rng, 6) + "-" * l2 + rand_seq(rng, 6)
    q1s = [crowded_queries(rng, u1, cap, 120) for cap in range(m1 + 1)]
    q2s = [crowded_queries(rng, u2, cap, 120) for cap in range(m2 + 1)]
    b1, b2 = [_bits(s, _SET_BITS) for s in u1], [_bits(s, _SET_BITS) for s in u2]

    def near(pool, bits, target, cap, tries=30):
        """a query whose unique hit within cap is `target` (at any distance), or the target itself"""
        want = pool.index(target)
        for _ in range(tries):
            d = rng.randint(0, cap)
            q = list(target)
            for s in _spread(rng, len(target), pool.positions, d, rng.randrange(24)):
                q[s] = rng.choice([b for b in BASES if b != target[s]])
            q = "".join(q)
            if crowded_outcome(bits, q, cap)[::2] == ("hit", want):
                return q
        return target

    reads1, reads2, probes = [], [], []
    for _ in range(n_reads):
        u = rng.random()
        c1, c2 = rng.choice([0, 0, 0, 1]) if m1 else 0, rng.choice([0, 0, 0, 1]) if m2 else 0
        cap1, cap2 = m1 - c1, m2 - c2
        if u < 0.25 and special and cap1 >= 1:
            k, p, r, t, x, y = rng.choice(special)
            c, alt, _ = u1.stars[k]
            d = rng.randint(1, cap1)
            q = list(c)
            q[p], q[r] = alt[p], alt[r]
            for s in _spread(rng, l1, u1.positions, d - 1, rng.randrange(24), fixed=(p, r, t)):
                q[s] = _third(rng, u1, k, s)
            if rng.random() < 0.3 and d < cap1:         # one arm nearer: a unique best pair
                q[r] = c[r]
            a = "".join(q)
            b = near(u2, b2, x if rng.random() < 0.6 else y, cap2)
        elif u < 0.45 and special and cap1 >= 1:        # at the centre: every arm of the star lies within the cap
            k, p, r, t, x, y = rng.choice(special)
            a = crowded_query(rng, u1, "centre", rng.randint(0, cap1 - 1), rng.randrange(24), star=k)
            b = near(u2, b2, rng.choice([x, y]), cap2)
        elif u < 0.8:
            x, y = rng.choice(rows)
            a, b = near(u1, b1, x, cap1), near(u2, b2, y, cap2)
        else:
            a, b = rng.choice(q1s[cap1]), rng.choice(q2s[cap2])
        probes.append((a, b))
        a, b = _embed(rng, t1, [a], c1, 8), _embed(rng, t2, [b], c2, 8)
        if l1 < CROWDED_SHORT and rng.random() < 0.1:       # a second construct on mate 1: first and best differ
            a += _embed(rng, t1, [near(u1, b1, rng.choice(rows)[0], m1)], 0, 0)
        if randomized and rng.random() < 0.5:
            a, b = b, a
        reads1.append(a)
        reads2.append(b)
    return dict(kind="dual", template1=t1, reverse1=False, mismatches1=m1, pool1=[a for a, _ in rows],
                template2=t2, reverse2=False, mismatches2=m2, pool2=[b for _, b in rows],
                randomized=randomized, use_first=use_first, reads1=reads1, reads2=reads2, probes=probes)


def crowded_dual_single_end_case(seed: int, lens: tuple, budget: int, use_first: bool = True, n_reads: int = 1500) -> dict:
    """countDualBarcodesSingleEnd (and its diagnostics form): the rows of a crowded pool of the combined length, cut into
    the regions -- a row that differs from its centre in one region shares the other region's barcode with it, so the
    barcodes of a region recur over several rows."""
    rng = random.Random(f"dual_single_end {seed} {lens} {budget}")
    total = sum(lens)
    pool = crowded_pool(rng, total, budget, iupac=False)
    cuts = [sum(lens[:i]) for i in range(len(lens) + 1)]

    def cut(s):
        return [s[a:b] for a, b in zip(cuts, cuts[1:])]
    pools = [list(col) for col in zip(*(cut(s) for s in pool))]
    template = rand_seq(rng, 8) + "".join("-" * n + rand_seq(rng, 5 if i + 1 < len(lens) else 8) for i, n in enumerate(lens))
    per_cap = [crowded_queries(rng, pool, cap, 120) for cap in range(budget + 1)]
    reads = []
    for _ in range(n_reads):
        c = rng.choice(list(range(budget + 1)) * 3 + [budget + 1])
        read = _embed(rng, template, cut(rng.choice(per_cap[max(budget - c, 0)])), c, 8)
        reads.append(rc(read) if rng.random() < 0.5 else read)
    return dict(kind="dual_single_end", template=template, strand=2, pools=pools, mismatches=budget, use_first=use_first, reads=reads)


# The crowded cases with a kaori golden (tests/golden/kaori_crowded.json, by name), one seed each.
CROWDED_MATCH_LENGTHS = (8, 20, 32, 33, 40, 64, 65, 128, 129, 192, 256)
CROWDED_MATCH_BUDGETS = (0, 1, 2, 3, 4, 5)
CROWDED_SINGLE_LENGTHS = (20, 40, 100)
CROWDED_SINGLE_BUDGETS = (1, 2, 3, 4)
CROWDED_COMBO_LENGTHS = ((12, 10), (40, 8))
CROWDED_COMBO_BUDGETS = (2, 4)
CROWDED_SEED = 20261018


def crowded_golden_cases() -> dict:
    """name -> zero-argument builder of every crowded match, single and combo case"""
    out = {}
    for length in CROWDED_MATCH_LENGTHS:
        for budget in CROWDED_MATCH_BUDGETS:
            for reverse in (False, True):
                out[f"match-{length}-{budget}-{'rev' if reverse else 'fwd'}"] = \
                    lambda a=length, b=budget, r=reverse: crowded_match_case(CROWDED_SEED, a, b, r)
    for length in CROWDED_SINGLE_LENGTHS:
        for budget in CROWDED_SINGLE_BUDGETS:
            for first in (True, False):
                out[f"single-{length}-{budget}-{'first' if first else 'best'}"] = \
                    lambda a=length, b=budget, f=first: crowded_single_case(CROWDED_SEED, a, b, f)
    for lens in CROWDED_COMBO_LENGTHS:
        for budget in CROWDED_COMBO_BUDGETS:
            out[f"combo-{lens[0]}x{lens[1]}-{budget}"] = lambda a=lens, b=budget: crowded_combo_case(CROWDED_SEED, a, b)
    return out
