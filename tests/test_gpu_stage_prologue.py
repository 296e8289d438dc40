"""The staged kernels' prologue at the shapes where its order of work and its unguarded loads can go wrong.

A workgroup issues its first round of 16-byte loads before anything else, fills the strand table (and the combination
kernels' pool descriptors) behind them on its last wavefront, loads a chunk index past the span's end from the span's
last chunk instead of guarding the load, issues a second round's loads between the first round's transposes, and takes
each seed's walks with one wide scalar load (csrc/scg_staged.hip.h: stage_reads, stage_tile, seed_candidates).  Every
batch here is counted by the staged kernels and compared exactly with the oracle (oracle/liboracle.so); one is also
compared with the byte-wise general kernels (SCG_FORCE_GENERAL=1), as the parity suite does.  160-base tiles hold
1 280 chunks a round (256 lanes x 5 loads), 320-base tiles 2 560.
"""
import random

import numpy as np
import pytest
import torch

from tests import gen

pytestmark = pytest.mark.gpu

C, V = "c", "v"
BOTH = 2                                     # strand: 0 forward, 1 reverse, 2 both


def _plan(seed, segs=((C, 10), (V, 12), (C, 10)), npool=40):
    rng = random.Random(seed)
    t = gen.segments_template(rng, list(segs))
    pools = [gen.make_pool(rng, npool, n, gen.BASES, min_dist=3) for kind, n in segs if kind == V]
    return rng, t, pools


def _read(rng, t, pools, length, strand=BOTH, p_sub=0.015):
    """A read of exactly `length` bases: a construct (now and then mutated, on either strand) at a random place when it
    fits, random bases otherwise."""
    if length < len(t) or rng.random() < 0.15:
        return gen.rand_seq(rng, length)
    core = gen.mutate(rng, gen.fill_template(t, [rng.choice(p) for p in pools]), p_sub, 0.004, 0.02)
    at = rng.choice((0, length - len(t), rng.randint(0, length - len(t))))
    read = gen.rand_seq(rng, at) + core + gen.rand_seq(rng, length - len(t) - at)
    if strand == 1 or (strand == BOTH and rng.random() < 0.5):
        read = gen.rc(read)
    return read


def _device_bytes(reads, gpu, shift=0):
    """The reads back to back on the device, the first `shift` bytes past a 16-byte boundary (torch allocates at
    multiples of 512), and their offsets."""
    bs = [r.encode() if isinstance(r, str) else bytes(r) for r in reads]
    offs = np.zeros(len(bs) + 1, dtype=np.int64)
    offs[1:] = np.cumsum([len(b) for b in bs])
    flat = np.frombuffer(b"\0" * shift + b"".join(bs) + b"\0", dtype=np.uint8).copy()
    big = torch.from_numpy(flat).to(gpu)
    seqs = big[shift:shift + int(offs[-1])] if offs[-1] else big[shift:shift + 1]
    assert seqs.data_ptr() % 16 == shift
    return seqs, torch.from_numpy(offs.astype(np.int32)).to(gpu), bs


def _count_single(sc, gpu, reads, t, strand, pool, mm, use_first=True, fixed_len=0, shift=0):
    seqs, offs, _ = _device_bytes(reads, gpu, shift)
    with sc.Plan.single(t, strand, pool, mm, use_first) as plan:
        if fixed_len:
            plan.count(seqs, None, fixed_len=fixed_len, n_reads=len(reads))
        else:
            plan.count(seqs, offs)
        return plan.read()


def _check_single(sc, oracle, gpu, reads, t, pool, mm, strand=BOTH, use_first=True, fixed_len=0, shift=0):
    exp = oracle.count_single(reads, t, strand, pool, mm, use_first)
    got = _count_single(sc, gpu, reads, t, strand, pool, mm, use_first, fixed_len, shift)
    assert got[1] == exp[1] == len(reads)
    assert np.array_equal(got[0], exp[0]), np.flatnonzero(got[0] != exp[0])
    return exp


@pytest.mark.parametrize("n", [1, 63, 64, 65, 255, 256, 257, 513])
def test_batch_sizes(sc, oracle, gpu, n):
    """150-base reads: a last workgroup with fewer chunks (10 for one read) than lanes, with one round only (63, 64, 65
    reads: 591 .. 610 chunks), with a second round (255, 256 and the first workgroups of 257 and 513) -- as a fixed-length
    batch and through offsets."""
    rng, t, (pool,) = _plan(100 + n)
    reads = [_read(rng, t, [pool], 150) for _ in range(n)]
    exp = _check_single(sc, oracle, gpu, reads, t, pool, 1, fixed_len=150)
    assert n < 60 or exp[0].sum() > n // 2
    _check_single(sc, oracle, gpu, reads, t, pool, 1)


@pytest.mark.parametrize("shift", [0, 1])
def test_second_round_of_one_chunk(sc, oracle, gpu, shift):
    """256 reads of 80 bases are 1 280 chunks, one round exactly; starting one byte past a 16-byte boundary the span has
    1 281 and the second round is lane 0's single chunk.  The same with 160 bases: 2 560 chunks and a third round of one."""
    for length in (80, 160):
        rng, t, (pool,) = _plan(200 + length)
        reads = [_read(rng, t, [pool], length) for _ in range(3 * 256)]
        _check_single(sc, oracle, gpu, reads, t, pool, 1, fixed_len=length, shift=shift)


@pytest.mark.parametrize("length", [20, 37, 150, 160])
def test_read_lengths(sc, oracle, gpu, length):
    """Fixed lengths from the template's own (T = 20) to the tile's 160, then the same reads among others of mixed
    lengths: shorter than the template, empty, and up to 160 bases."""
    rng, t, (pool,) = _plan(300 + length, ((C, 4), (V, 12), (C, 4)))
    assert len(t) == 20
    reads = [_read(rng, t, [pool], length) for _ in range(300)]
    _check_single(sc, oracle, gpu, reads, t, pool, 1, fixed_len=length)
    mixed = []
    for r in reads:
        mixed.append(r)
        mixed.append(_read(rng, t, [pool], rng.choice((0, 0, 7, 19, 20, 21, 37, 150, 160))))
    assert any(len(r) == 0 for r in mixed) and any(0 < len(r) < len(t) for r in mixed)
    _check_single(sc, oracle, gpu, mixed, t, pool, 1)
    _check_single(sc, oracle, gpu, [""] * 5 + mixed[:40] + [""] * 300, t, pool, 1)      # (a workgroup of no bytes at all)


@pytest.mark.parametrize("shift", [1, 7, 15])
def test_misaligned_base(sc, oracle, gpu, shift):
    """The read buffer starts 1, 7 and 15 bytes past a 16-byte boundary: the first tile begins before its first read, so
    the first and the last workgroup take the guarded path and the one between them the unguarded one, with a span that
    starts inside a chunk."""
    rng, t, (pool,) = _plan(400 + shift)
    reads = [_read(rng, t, [pool], 150) for _ in range(600)]
    _check_single(sc, oracle, gpu, reads, t, pool, 1, fixed_len=150, shift=shift)
    mixed = [r[:rng.choice((150, 150, 149, 133, 40, 0))] for r in reads]
    _check_single(sc, oracle, gpu, mixed, t, pool, 1, shift=shift)


@pytest.mark.parametrize("odd", [b"N", b"n", b"R", b"\n"])
def test_nonstandard_bytes_at_edges(sc, oracle, gpu, odd):
    """A byte that is no base as the first and the last byte of the buffer, of a workgroup's span and of a 16-byte chunk,
    each inside a construct (constant base or barcode), in an otherwise standard batch: the chunk's validity bits come
    from the slow path of one wavefront only."""
    rng, t, (pool,) = _plan(500 + odd[0])
    length, n = 150, 3 * 256 + 5

    def construct_read(at_end):
        core = gen.fill_template(t, [rng.choice(pool)])
        pad = gen.rand_seq(rng, length - len(t))
        return pad + core if at_end else core + pad

    reads = [construct_read(i % 2 == 1).encode() for i in range(n)]      # even reads open with a construct, odd ones end with one
    flat = bytearray(b"".join(reads))
    spots = [0, len(flat) - 1,                                   # the buffer
             256 * length - 1, 256 * length, 512 * length - 1, 512 * length,      # workgroup spans
             15, 16, 256 * length + 31, 256 * length + 32,       # chunks
             2 * length + 5, 2 * length + 12]                    # a constant base and a barcode base inside one construct
    for s in spots:
        flat[s:s + 1] = odd
    reads = [bytes(flat[i * length:(i + 1) * length]) for i in range(n)]
    exp = _check_single(sc, oracle, gpu, reads, t, pool, 1, fixed_len=length)
    assert n - 12 <= exp[0].sum() < n                            # (a read with two of them is lost, one with one mostly not)
    _check_single(sc, oracle, gpu, reads, t, pool, 1, shift=7)


PLANS = {
    # name: (segments, mismatches, strand) -- where the pigeonhole seeds of the constant bases fall (template positions
    # 0-31 are block 0, 32-63 block 1) and how many there are (mismatches + 1 per strand)
    "block0_mm1": (((C, 10), (V, 12), (C, 10)), 1, BOTH),            # T = 32: both flanks in block 0
    "block1_mm0": (((C, 2), (V, 30), (C, 20)), 0, BOTH),             # the one seed lies in positions 32-51
    "both_blocks_mm1": (((C, 10), (V, 24), (C, 10)), 1, BOTH),       # T = 44: one flank per block
    "three_seeds_mm2": (((C, 16), (V, 16), (C, 16)), 2, BOTH),
    "reverse_only_mm1": (((C, 10), (V, 24), (C, 10)), 1, 1),
    "forward_only_mm0": (((C, 12), (V, 12), (C, 3)), 0, 0),
}


@pytest.mark.parametrize("name", sorted(PLANS))
@pytest.mark.parametrize("use_first", [True, False])
def test_seed_walks(sc, oracle, gpu, monkeypatch, name, use_first):
    """Every seed-walk length the one wide scalar load has to hold: seeds in block 0, block 1 and both, one to three seeds
    a strand, one strand or both -- staged against the oracle, and the general kernels against the same."""
    segs, mm, strand = PLANS[name]
    rng, t, (pool,) = _plan(name, segs)
    assert gen.compact_ok(t, mm)
    reads = [_read(rng, t, [pool], 100, strand if strand != 1 else BOTH, p_sub=0.05) for _ in range(520)]
    _check_single(sc, oracle, gpu, reads, t, pool, mm, strand, use_first, fixed_len=100)
    monkeypatch.setenv("SCG_FORCE_GENERAL", "1")
    _check_single(sc, oracle, gpu, reads, t, pool, mm, strand, use_first, fixed_len=100)


def test_seed_of_one_base(sc, oracle, gpu):
    """Flanks that are runs of one base: all steps of a seed lie in one code's walk (ten of them, three walk words), the
    other three walks are empty."""
    rng = random.Random(600)
    t = "A" * 10 + "-" * 12 + "C" * 10
    pool = gen.make_pool(rng, 40, 12, gen.BASES, min_dist=3)
    reads = [_read(rng, t, [pool], 100, p_sub=0.05) for _ in range(520)]
    _check_single(sc, oracle, gpu, reads, t, pool, 1, fixed_len=100)
    _check_single(sc, oracle, gpu, reads, t, pool, 1, use_first=False)


def test_combination_plan(sc, oracle, gpu):
    """The combination kernel: its two pool descriptors reach LDS on the fill wavefront behind the first loads."""
    rng, t, pools = _plan(700, ((C, 8), (V, 8), (C, 6), (V, 10), (C, 8)), npool=20)
    reads = [_read(rng, t, pools, 150) for _ in range(513)]
    exp = oracle.count_combo(reads, t, BOTH, pools[0], pools[1], 1, True)
    for shift in (0, 7):
        seqs, offs, _ = _device_bytes(reads, gpu, shift)
        with sc.Plan.combo(t, BOTH, pools[0], pools[1], 1, True) as plan:
            plan.count(seqs, None, fixed_len=150, n_reads=len(reads))
            got = plan.read_combo()
        assert got[2] == exp[2] == len(reads)
        assert np.array_equal(got[0], exp[0]) and np.array_equal(got[1], exp[1])
    assert exp[1].sum() > 200


@pytest.mark.parametrize("shift", [0, 7])
def test_320_base_tiles(sc, oracle, gpu, shift):
    """NW = 10: ten loads a lane and round, the general seed scanner.  256 reads of 320 bases are two rounds exactly; from
    a shifted base the span has a third round of one chunk."""
    rng, t, (pool,) = _plan(800)
    reads = [_read(rng, t, [pool], 320) for _ in range(2 * 256 + 9)]
    _check_single(sc, oracle, gpu, reads, t, pool, 1, fixed_len=320, shift=shift)
    mixed = [r[:rng.choice((320, 319, 161, 31, 0))] for r in reads]
    _check_single(sc, oracle, gpu, mixed, t, pool, 1, shift=shift)
