"""The device compaction of a dense combination histogram (csrc/scg_combine.hip) through scg_combo_compact_device, against
np.flatnonzero (tests/combo_matrix_ref.py) and against the host's scg_combo_compact: the same 2 x K indices in cell order and
the same K counts, at every size at which a tile, a wave or a 16-byte load begins, ends or is cut short, in grids that make
the decode of a cell number into (first, second) wrap at every kind of row end.

T is the tile of the kernels in cells, read from the header that defines it, so that a retune moves the sizes with it."""
import numpy as np
import pytest

from tests import combo_matrix_ref as ref

pytestmark = pytest.mark.gpu

T = ref.tile_cells()
INT32_MAX = 2**31 - 1
TOTALS = [1, 63, 64, 65, 255, 256, 257, T - 1, T, T + 1, 2 * T - 1, 2 * T, 2 * T + 1, 1024 * T + 3]
PATTERNS = ["all zero", "all non-zero", "first cell", "last cell", "last cell of every tile", "every other cell", "1 %", "50 %"]


def grids(total):
    """(1, N), (N, 1) and, where N factors that way, both pools above 1 with n1 not a power of two (the largest such n1 up
    to the square root, else the smallest)."""
    out = [(1, total), (total, 1)]
    odd = [d for d in range(3, int(total**0.5) + 1) if total % d == 0 and d & (d - 1)]
    if not odd:
        odd = [total // d for d in range(2, int(total**0.5) + 1) if total % d == 0 and (total // d) & (total // d - 1)][-1:]
    if odd:
        out.append((total // odd[-1], odd[-1]))
    return out


def counts_for(rng, n):
    """n non-zero counts: 1 and INT32_MAX among ordinary ones."""
    c = rng.integers(1, 1000, size=n, dtype=np.int64)
    c[rng.random(n) < 0.2] = 1
    c[rng.random(n) < 0.2] = INT32_MAX
    if n:
        c[0], c[-1] = INT32_MAX, 1
    return c.astype(np.int32)


def cells_of(pattern, total, seed):
    rng = np.random.default_rng(seed)
    if pattern == "all zero":
        at = np.zeros(0, dtype=np.int64)
    elif pattern == "all non-zero":
        at = np.arange(total)
    elif pattern == "first cell":
        at = np.array([0])
    elif pattern == "last cell":
        at = np.array([total - 1])
    elif pattern == "last cell of every tile":           # (of the cut-short last tile too)
        at = np.unique(np.append(np.arange(T - 1, total, T), total - 1))
    elif pattern == "every other cell":
        at = np.arange(seed % 2, total, 2)
    else:
        at = np.flatnonzero(rng.random(total) < (0.01 if pattern == "1 %" else 0.5))
    cells = np.zeros(total, dtype=np.int32)
    cells[at] = counts_for(rng, len(at))
    return cells


def check(sc, cells, n0, n1):
    exp_idx, exp_freq = ref.compact(cells, n0, n1)
    got_idx, got_freq = sc.combo_compact_device(cells, n0, n1)
    assert got_idx.dtype == np.int32 and got_freq.dtype == np.int32
    assert got_idx.shape == exp_idx.shape and got_freq.shape == exp_freq.shape, (got_idx.shape, exp_idx.shape)
    assert np.array_equal(got_freq, exp_freq)
    assert np.array_equal(got_idx, exp_idx)
    host_idx, host_freq = sc.combo_compact(cells, n0, n1)
    assert np.array_equal(got_idx, host_idx) and np.array_equal(got_freq, host_freq)


def test_the_factored_grids_exercise_the_decode():
    """(no device needed) Every total that has such a factorisation gets a grid with both pools above 1 and n1 not a power
    of two; the totals without one are the powers of two and the primes."""
    with_third = {t for t in TOTALS if len(grids(t)) == 3}
    assert {63, 65, 255, T - 1, T + 1, 2 * T + 1} <= with_third
    for t in with_third:
        n0, n1 = grids(t)[2]
        assert n0 > 1 and n1 > 1 and n0 * n1 == t and n1 & (n1 - 1)


@pytest.mark.parametrize("total", TOTALS)
def test_compaction_matches_flatnonzero_and_the_host(sc, gpu, total):
    for pattern in PATTERNS:
        cells = cells_of(pattern, total, seed=total % 1000 + len(pattern))
        for n0, n1 in grids(total):
            check(sc, cells, n0, n1)


def test_the_dense_limit(sc, gpu):
    """Exactly 2^26 cells, the default dense limit: the first cell, the last cell and about a thousand others."""
    n0 = n1 = 8192
    rng = np.random.default_rng(26)
    at = np.unique(np.concatenate([[0, n0 * n1 - 1], rng.integers(0, n0 * n1, size=1000)]))
    cells = np.zeros(n0 * n1, dtype=np.int32)
    cells[at] = counts_for(rng, len(at))
    check(sc, cells, n0, n1)


def test_empty_grids(sc, gpu):
    for n0, n1 in ((0, 5), (5, 0), (0, 0)):
        idx, freq = sc.combo_compact_device(np.zeros(0, dtype=np.int32), n0, n1)
        assert idx.shape == (2, 0) and freq.shape == (0,)
