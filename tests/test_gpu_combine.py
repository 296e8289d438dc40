"""scg_combine_combinations: combineComboCounts (R/combineComboCounts.R:31-57) on the device -- the union of the files'
combinations by radix sort and run-length encode, and every entry's row by a lower bound over the distinct keys -- against
the numpy restatement of tests/combo_matrix_ref.py and, for the small cases, against the dictionary loop of
tests/rlevel.py::combineComboCounts."""
import numpy as np
import pytest

from tests import combo_matrix_ref as ref
from tests import rlevel

pytestmark = pytest.mark.gpu

INT32_MAX = 2**31 - 1
EMPTY = (np.zeros((2, 0), dtype=np.int32), np.zeros(0, dtype=np.int32))


def unique_list(rng, k, pool=(1000, 1000), sort=False, counts=None):
    """One file's list: k distinct combinations of pool[0] x pool[1], in random order unless `sort`."""
    cells = rng.choice(pool[0] * pool[1], size=k, replace=False)
    if sort:
        cells = np.sort(cells)
    idx = np.stack([cells // pool[1], cells % pool[1]]).astype(np.int32)
    freq = rng.integers(1, 10000, size=k).astype(np.int32) if counts is None else np.asarray(counts, dtype=np.int32)
    return idx, freq


def draws(rng, npool, nreads):
    """GENERATOR of tests/testthat/test-combo-combine.R: nreads draws of two indices out of npool, tabulated."""
    x, y = rng.integers(0, npool, size=nreads), rng.integers(0, npool, size=nreads)
    cells, freq = np.unique(x * npool + y, return_counts=True)
    return np.stack([cells // npool, cells % npool]).astype(np.int32), freq.astype(np.int32)


def second_reference(lists):
    """tests/rlevel.py::combineComboCounts on the same lists (1-based indices there)."""
    results = [rlevel.ComboCounts(names=["first", "second"], combinations={"first": (i[0].astype(np.int64) + 1).tolist(), "second": (i[1].astype(np.int64) + 1).tolist()},
                                  counts=f, nreads=0) for i, f in lists]
    combos, mat = rlevel.combineComboCounts(*results)
    idx = np.array([combos["first"], combos["second"]], dtype=np.int64).reshape(2, -1) - 1
    return idx.astype(np.int32), mat


def check(sc, lists, small=True):
    expected = ref.combine(lists)
    got = sc.combine_combinations(lists)
    ref.assert_matrix(got, expected)
    if small:
        ref.assert_matrix(got, second_reference(lists))
    return got


def test_no_files_and_empty_files(sc, gpu):
    rng = np.random.default_rng(1)
    a, b = unique_list(rng, 7), unique_list(rng, 12)
    check(sc, [])
    check(sc, [EMPTY])
    check(sc, [EMPTY, EMPTY, EMPTY])
    check(sc, [EMPTY, a, b])
    check(sc, [a, EMPTY, b])
    check(sc, [a, b, EMPTY])
    check(sc, [EMPTY, a, EMPTY, EMPTY, b, EMPTY])


def test_one_file_identical_files_disjoint_files(sc, gpu):
    rng = np.random.default_rng(2)
    a = unique_list(rng, 40)
    idx, matrix = check(sc, [a])
    assert matrix.shape == (40, 1)
    idx, matrix = check(sc, [a, a, a])
    assert matrix.shape == (40, 3) and np.array_equal(matrix[:, 0], matrix[:, 2])
    lo, hi = unique_list(rng, 30, pool=(10, 50)), unique_list(rng, 30, pool=(10, 50))
    hi[0][0] += 10                                          # no first index in common
    idx, matrix = check(sc, [lo, hi])
    assert matrix.shape == (60, 2) and not (matrix[:, 0] * matrix[:, 1]).any()


@pytest.mark.parametrize("nreads", [1, 5, 10, 50, 100, 500])
def test_three_samples_of_the_reference_test(sc, gpu, nreads):
    rng = np.random.default_rng(1000 + nreads)
    check(sc, [draws(rng, 10, nreads) for _ in range(3)])


def test_unsorted_lists_and_explicit_zero_counts(sc, gpu):
    rng = np.random.default_rng(3)
    lists = [unique_list(rng, 200, pool=(30, 30)) for _ in range(4)]
    lists.append(tuple(x[..., ::-1] for x in unique_list(rng, 100, pool=(30, 30), sort=True)))     # descending
    check(sc, lists)
    # a combination counted zero times keeps its row, in a file of its own and next to counted ones
    zero = (np.array([[3, 5], [4, 0]], dtype=np.int32), np.array([0, 0], dtype=np.int32))
    mixed = (np.array([[3, 1, 9], [4, 1, 9]], dtype=np.int32), np.array([0, 7, 0], dtype=np.int32))
    idx, matrix = check(sc, [zero, mixed])
    assert idx.T.tolist() == [[1, 1], [3, 4], [5, 0], [9, 9]] and matrix.tolist() == [[0, 7], [0, 0], [0, 0], [0, 0]]


def test_the_ends_of_the_index_range(sc, gpu):
    corners = np.array([[0, 0, INT32_MAX, INT32_MAX, 1, INT32_MAX - 1], [0, INT32_MAX, 0, INT32_MAX, INT32_MAX - 1, 1]], dtype=np.int32)
    freq = np.array([1, 2, 3, INT32_MAX, 5, 6], dtype=np.int32)
    idx, matrix = check(sc, [(corners, freq), (corners[:, ::-1], freq), (corners[:, [3, 0]], freq[:2])])
    assert idx[:, 0].tolist() == [0, 0] and idx[:, -1].tolist() == [INT32_MAX, INT32_MAX]
    assert matrix[-1].tolist() == [INT32_MAX, 3, 1]


@pytest.mark.parametrize("n", [255, 256, 257, 65537])
def test_entries_at_the_launch_boundaries(sc, gpu, n):
    """N entries in all (one lane per entry, 256 lanes per workgroup), split over three files of unequal length."""
    rng = np.random.default_rng(n)
    a, b = n // 3, n // 2
    lists = [unique_list(rng, k, pool=(500, 400)) for k in (a, b - a, n - b)]
    check(sc, lists, small=n < 1000)


@pytest.mark.parametrize("k", [1, 2, 255, 256, 257, 65535, 65536, 65537])
def test_distinct_keys_at_the_powers_of_two(sc, gpu, k):
    """K distinct combinations in the union (the lower bound halves K down to one): every one of them in some file, the
    first and the last in all three."""
    rng = np.random.default_rng(k)
    cells = np.sort(rng.choice(3000 * 700, size=k, replace=False))
    lists = []
    for f in range(3):
        take = np.flatnonzero((np.arange(k) % 3 == f) | (np.arange(k) == 0) | (np.arange(k) == k - 1))
        take = rng.permutation(take)
        lists.append((np.stack([cells[take] // 700, cells[take] % 700]).astype(np.int32), rng.integers(1, 99, size=len(take)).astype(np.int32)))
    idx, matrix = check(sc, lists, small=k < 1000)
    assert matrix.shape == (k, 3)


def test_a_repeat_within_one_file_is_the_references_error(sc, gpu):
    from screencounter_amd import _lib
    rng = np.random.default_rng(4)
    clean = [unique_list(rng, 300, pool=(40, 40)) for _ in range(3)]
    idx, freq = unique_list(rng, 300, pool=(40, 40), sort=True)

    def with_repeat(at, of):
        i = idx.copy()
        i[:, at] = i[:, of]
        return i, freq

    cases = {
        "adjacent": [with_repeat(11, 10), clean[0]],
        "far apart": [clean[0], with_repeat(299, 0), clean[1]],
        "last file only": [clean[0], clean[1], clean[2], with_repeat(150, 7)],
        "only file": [with_repeat(1, 0)],
        "two entries": [(np.array([[5, 5], [6, 6]], dtype=np.int32), np.array([1, 2], dtype=np.int32))],
    }
    for name, lists in cases.items():
        with pytest.raises(ValueError, match="unique within each DataFrame"):
            ref.combine(lists)
        with pytest.raises(sc.ScgError) as e:
            sc.combine_combinations(lists)
        assert (e.value.code, str(e.value)) == (_lib.SCG_ERR_INVALID, ref.DUPLICATED), name
    # the same combination in two files is what the function is for
    check(sc, [clean[0], clean[0]])


def test_a_negative_index_is_refused(sc, gpu):
    from screencounter_amd import _lib
    for bad in ([[1, -1], [2, 3]], [[1, 2], [3, -2147483648]]):
        with pytest.raises(sc.ScgError) as e:
            sc.combine_combinations([(np.array([[0], [0]], dtype=np.int32), np.array([1], dtype=np.int32)),
                                     (np.array(bad, dtype=np.int32), np.array([1, 1], dtype=np.int32))])
        assert e.value.code == _lib.SCG_ERR_INVALID


def test_device_lists(sc, gpu):
    """The union runs on the first device of the call's list."""
    rng = np.random.default_rng(5)
    lists = [unique_list(rng, 50, pool=(20, 20)) for _ in range(3)]
    expected = ref.combine(lists)
    for devices in (None, [0], [0, 0, 0]):
        ref.assert_matrix(sc.combine_combinations(lists, devices), expected)
