"""An independent restatement of combineComboCounts (R/combineComboCounts.R:31-57) in numpy, for the tests of the
combination-matrix entries: bind the lists, order by (first, second), keep one row per distinct combination, and put every
list's counts into its column at the rows of its combinations.  Nothing here calls the library."""
import os
import re

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DUPLICATED = "barcode combinations should be unique within each DataFrame in '...'"      # R/combineComboCounts.R:51


def tile_cells() -> int:
    """The tile of the device compaction, in cells, as the header of the launchers defines it."""
    text = open(os.path.join(ROOT, "screencounter_amd", "csrc", "scg_launch.h")).read()
    return int(re.search(r"^#define\s+SCG_COMPACT_TILE_CELLS\s+(\d+)\s*$", text, re.M).group(1))


def keys_of(indices) -> np.ndarray:
    idx = np.asarray(indices, dtype=np.int64).reshape(2, -1)
    return (idx[0] << 32) | idx[1]


def combine(lists):
    """lists: per file (indices [2, K_f], freq [K_f]) in any order -> (indices int32[2, K] sorted by (first, second),
    matrix int32[K, n_files]).  ValueError(DUPLICATED) when a combination appears twice within one list."""
    n = len(lists)
    per_file = [keys_of(i) for i, _ in lists]
    for k in per_file:
        if len(np.unique(k)) != len(k):
            raise ValueError(DUPLICATED)
    union = np.unique(np.concatenate(per_file)) if n else np.zeros(0, dtype=np.int64)
    matrix = np.zeros((len(union), n), dtype=np.int32)
    for f, (k, (_, freq)) in enumerate(zip(per_file, lists)):
        matrix[np.searchsorted(union, k), f] = np.asarray(freq, dtype=np.int32).reshape(-1)
    indices = np.stack([union >> 32, union & 0xFFFFFFFF]).astype(np.int32) if len(union) else np.zeros((2, 0), dtype=np.int32)
    return indices, matrix


def compact(cells: np.ndarray, n0: int, n1: int):
    """Dense cells -> (indices int32[2, K], freq int32[K]) by np.flatnonzero: cell c is (c // n1, c % n1)."""
    flat = np.asarray(cells).reshape(-1)[:n0 * n1]
    at = np.flatnonzero(flat)
    return np.stack([at // n1, at % n1]).astype(np.int32).reshape(2, -1), flat[at].astype(np.int32)


def assert_matrix(got, expected):
    (gi, gm), (ei, em) = got, expected
    assert gi.dtype == np.int32 and gm.dtype == np.int32
    assert gi.shape == ei.shape and gm.shape == em.shape, (gi.shape, ei.shape, gm.shape, em.shape)
    assert np.array_equal(gi, ei)
    assert np.array_equal(gm, em)
