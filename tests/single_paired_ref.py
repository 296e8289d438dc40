"""kaori::SingleBarcodePairedEnd (handlers/SingleBarcodePairedEnd.hpp:93-124) composed from the single-end oracle, one read
at a time: what the seeded tests of the paired single-barcode handler compare against.  tests/golden/kaori_single_paired.json
(the real handler's outputs) pins the composition: test_single_paired_reference_cpu.py.

First mode: the index of mate 1 at the full budget, else of mate 2.  Best mode: a read's (index, mismatches) is what
search_best counts at the smallest budget at which it counts anything -- at a smaller budget nothing is within reach, at a
larger one the fewest mismatches stay the same -- and the handler's rule is applied to the two mates' results.
About 1.4 ms per pair: keep callers at 1 500 pairs or fewer."""
import random

import numpy as np

from tests import gen


def make_mates(rng: random.Random, reads):
    """Mate 2 for a single-end case's reads: the same reads shuffled, so that both mates carry barcodes (mostly different
    ones); every third one mate 1 read again with fresh substitutions (the same barcode, equal or unequal mismatches)."""
    mates = list(reads)
    rng.shuffle(mates)
    for k in range(0, len(reads), 3):
        mates[k] = gen.mutate(rng, reads[k], 0.02, 0, 0)
    return mates


def paired_case(rng: random.Random, **kwargs) -> dict:
    c = gen.random_single_case(rng, **kwargs)
    c["kind"] = "single_paired"
    c["reads1"] = c.pop("reads")
    c["reads2"] = make_mates(rng, c["reads1"])
    return c


def _one(oracle, read, template, strand, pool, budget, use_first):
    counts, _ = oracle.count_single([read], template, strand, pool, budget, use_first)
    hit = np.flatnonzero(counts)
    return int(hit[0]) if len(hit) else -1


def best_of_read(oracle, read, template, strand, pool, mismatches):
    """(index, mismatches) of search_best on one read, or (-1, None)."""
    for budget in range(mismatches + 1):
        i = _one(oracle, read, template, strand, pool, budget, False)
        if i >= 0:
            return i, budget
    return -1, None


def pair_index(oracle, a, b, template, strand, pool, mismatches, use_first):
    """The pool index the handler counts for the pair (a, b), or -1."""
    if use_first:                                                     # :94-99
        i = _one(oracle, a, template, strand, pool, mismatches, True)
        return i if i >= 0 else _one(oracle, b, template, strand, pool, mismatches, True)
    i1, m1 = best_of_read(oracle, a, template, strand, pool, mismatches)      # :100-121
    i2, m2 = best_of_read(oracle, b, template, strand, pool, mismatches)
    if i1 < 0 or i2 < 0:
        return max(i1, i2)
    if m1 != m2:
        return i1 if m1 < m2 else i2
    return i1 if i1 == i2 else -1


def count_single_paired(oracle, reads1, reads2, template, strand, pool, mismatches, use_first):
    """(counts int32[len(pool)], total).  Raises the oracle's error for arguments the reference rejects."""
    from oracle.pyoracle import OracleError
    if len(reads1) != len(reads2):
        raise OracleError("different number of reads in paired FASTQ files")
    oracle.count_single([], template, strand, pool, mismatches, use_first)     # the handler's argument checks
    counts = np.zeros(len(pool), dtype=np.int32)
    for a, b in zip(reads1, reads2):
        i = pair_index(oracle, a, b, template, strand, pool, mismatches, use_first)
        if i >= 0:
            counts[i] += 1
    return counts, len(reads1)
