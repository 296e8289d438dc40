"""Host-side mirror of the reference's operator interface for the hot path, at the Rcpp level.

Same names, positional arguments and return tuples as the functions R reaches through ``.Call`` (R/RcppExports.R:4-26
of the reference): ``count_single_barcodes``, ``count_combo_barcodes_single``, ``count_dual_barcodes``,
``match_barcodes``, their siblings and the many-files entries -- 0-based indices, int32 counts, scalar totals, exactly
what the ``Rcpp::List`` results hold.  The R functions above that level (R/count*.R) stay what they are in the
reference and are not part of this package; the tests keep a small mirror of them (tests/rlevel.py) so that the
reference's own test vectors can be written the way its tests write them.

Everything is computed by libscg on the GPU; errors the reference raises as R errors surface as ``ScgError``.

Every function reads: checks the reference makes before anything else, the outputs, the native call, the result's shape.
The marshalling steps are _lib's (pools, combinations, sequence blobs); what the many-files entries share is
_files_call and _files_counts below.
"""
from __future__ import annotations

import contextlib
import ctypes as C
import os
from typing import Sequence

import numpy as np

from . import _lib
from ._lib import ERRCAP, ScgError, check, combo_outputs, cstr_array, cstr_matrix, errbuf, i32_p, per_file_combo_outputs

TWO_REGIONS = "currently expecting only 2 variable regions for single-end combinatorial barcodes"   # src/count_combo_barcodes_single.cpp:44-46
SAME_LENGTH = "both barcode pools should be of the same length"                                     # kaori/handlers/DualBarcodesPairedEnd.hpp:106-109


def _int32_out(n: int):
    """A caller-allocated int32[n] output -> (the array, its pointer for the call); the result is `array[:n].copy()`."""
    out = np.zeros(max(n, 1), dtype=np.int32)
    return out, out.ctypes.data_as(i32_p)


def _path(path) -> bytes:
    return os.fspath(path).encode()


# =============================================================================================
# Rcpp level: one file (or one pair of files)
# =============================================================================================
def count_single_barcodes(path: str, constant: str, strand: int, pool: Sequence[str], mismatches: int,
                          use_first: bool, nthreads: int = 1):
    """src/count_single_barcodes.cpp:28-50 -> (counts int32[len(pool)], total)."""
    L, err = _lib.load(), errbuf()
    (counts, counts_p), total = _int32_out(len(pool)), C.c_int32(0)
    check(L.scg_count_single_barcodes(_path(path), constant.encode(), int(strand), *_lib.pool(pool),
                                      int(mismatches), int(bool(use_first)), int(nthreads), counts_p, C.byref(total), err, ERRCAP), err)
    return counts[:len(pool)].copy(), int(total.value)


def count_combo_barcodes_single(path: str, constant: str, strand: int, pool: Sequence[Sequence[str]], mismatches: int,
                                use_first: bool, nthreads: int = 1):
    """src/count_combo_barcodes_single.cpp:39-70 -> (indices int32[2, K] 0-based, freq int32[K], total)."""
    if len(pool) != 2:
        raise ScgError(_lib.SCG_ERR_INVALID, TWO_REGIONS)
    L, err = _lib.load(), errbuf()
    total = C.c_int32(0)
    with combo_outputs(L) as (combos, take):
        check(L.scg_count_combo_barcodes_single(_path(path), constant.encode(), int(strand), *_lib.pool(pool[0]), *_lib.pool(pool[1]),
                                                int(mismatches), int(bool(use_first)), int(nthreads), *combos, C.byref(total), err, ERRCAP), err)
        idx, freq = take()
    return idx, freq, int(total.value)


def count_combo_barcodes_regions(path: str, constant: str, strand: int, pools: Sequence[Sequence[str]], mismatches: int,
                                 use_first: bool, nthreads: int = 1):
    """Combinations over len(pools) variable regions (kaori::CombinatorialBarcodesSingleEnd for any number of regions, 1 to 8
    here) -> (indices int32[len(pools), K] 0-based, sorted by (first, ..., last), freq int32[K], total)."""
    L, err = _lib.load(), errbuf()
    total = C.c_int32(0)
    rows, sizes, _keep = _lib.cstr_matrix(pools)
    with combo_outputs(L, max(len(pools), 1)) as (combos, take):
        check(L.scg_count_combo_barcodes_regions(_path(path), constant.encode(), int(strand), rows, sizes, len(pools),
                                                 int(mismatches), int(bool(use_first)), int(nthreads), *combos, C.byref(total), err, ERRCAP), err)
        idx, freq = take()
    return idx, freq, int(total.value)


def count_single_barcodes_paired(path1: str, path2: str, constant: str, strand: int, pool: Sequence[str], mismatches: int, use_first: bool,
                                 nthreads: int = 1):
    """kaori::SingleBarcodePairedEnd (handlers/SingleBarcodePairedEnd.hpp:93-124) over two files: the barcode of a pair is
    looked for on either mate -> (counts int32[len(pool)], total pairs)."""
    L, err = _lib.load(), errbuf()
    (counts, counts_p), total = _int32_out(len(pool)), C.c_int32(0)
    check(L.scg_count_single_barcodes_paired(_path(path1), _path(path2), constant.encode(), int(strand), *_lib.pool(pool),
                                             int(mismatches), int(bool(use_first)), int(nthreads), counts_p, C.byref(total), err, ERRCAP), err)
    return counts[:len(pool)].copy(), int(total.value)


def count_dual_barcodes(path1: str, constant1: str, reverse1: bool, mismatches1: int, pool1: Sequence[str],
                        path2: str, constant2: str, reverse2: bool, mismatches2: int, pool2: Sequence[str],
                        randomized: bool, use_first: bool, diagnostics: bool = False, nthreads: int = 1):
    """src/count_dual_barcodes.cpp:74-117 -> (counts int32[n pairs], total), or with diagnostics=True the
    five outputs of the include.invalid=TRUE branch: (counts, (indices int32[2, K] 0-based, freq), total,
    barcode1_only, barcode2_only)."""
    if len(pool1) != len(pool2):
        raise ScgError(_lib.SCG_ERR_INVALID, SAME_LENGTH)
    L, err = _lib.load(), errbuf()
    (counts, counts_p), total = _int32_out(len(pool1)), C.c_int32(0)
    sides = (_path(path1), constant1.encode(), int(bool(reverse1)), int(mismatches1), cstr_array(pool1)[0],
             _path(path2), constant2.encode(), int(bool(reverse2)), int(mismatches2), cstr_array(pool2)[0], len(pool1))
    if diagnostics:
        b1, b2 = C.c_int32(0), C.c_int32(0)
        with combo_outputs(L) as (combos, take):
            check(L.scg_count_dual_barcodes_diagnostics(*sides, int(bool(randomized)), int(bool(use_first)), int(nthreads), counts_p, *combos,
                                                        C.byref(total), C.byref(b1), C.byref(b2), err, ERRCAP), err)
            invalid = take()
        return counts[:len(pool1)].copy(), invalid, int(total.value), int(b1.value), int(b2.value)
    check(L.scg_count_dual_barcodes(*sides, int(bool(randomized)), int(bool(use_first)), int(bool(diagnostics)), int(nthreads),
                                    counts_p, C.byref(total), err, ERRCAP), err)
    return counts[:len(pool1)].copy(), int(total.value)


def count_random_barcodes(path: str, constant: str, strand: int, mismatches: int, use_first: bool, nthreads: int = 1):
    """src/count_random_barcodes.cpp:41-62 -> ((sequences list[str] sorted, freq int32[K]), total)."""
    L, err = _lib.load(), errbuf()
    seq_p, freq_p = C.c_void_p(), i32_p()
    k, vlen, total = C.c_int64(0), C.c_int32(0), C.c_int32(0)
    check(L.scg_count_random_barcodes(_path(path), constant.encode(), int(strand), int(mismatches), int(bool(use_first)),
                                      int(nthreads), C.byref(seq_p), C.byref(freq_p), C.byref(k), C.byref(vlen), C.byref(total), err, ERRCAP), err)
    K = int(k.value)
    try:
        seqs = _lib.decode_sequences(seq_p, K, int(vlen.value))
        freq = np.ctypeslib.as_array(freq_p, shape=(max(K, 1),))[:K].copy()
    finally:
        L.scg_free(seq_p)
        L.scg_free(freq_p)
    return (seqs, freq), int(total.value)


def count_dual_barcodes_single_end(path: str, constant: str, pools: Sequence[Sequence[str]], strand: int, mismatches: int,
                                   use_first: bool, diagnostics: bool = False, nthreads: int = 1):
    """src/count_dual_barcodes_single_end.cpp:53-87 -> (counts int32[n combinations], total), or with diagnostics=True
    (counts, (indices int32[2, K] 0-based, freq), total) as in its include.invalid=TRUE branch."""
    L, err = _lib.load(), errbuf()
    nch = len(pools[0]) if pools else 0
    (counts, counts_p), total = _int32_out(nch), C.c_int32(0)
    rows, sizes, _keep = cstr_matrix(pools)
    if diagnostics:
        with combo_outputs(L) as (combos, take):
            check(L.scg_count_dual_barcodes_single_end_diagnostics(_path(path), constant.encode(), rows, sizes, len(pools), int(strand),
                                                                   int(mismatches), int(bool(use_first)), int(nthreads), counts_p, *combos,
                                                                   C.byref(total), err, ERRCAP), err)
            invalid = take()
        return counts[:nch].copy(), invalid, int(total.value)
    check(L.scg_count_dual_barcodes_single_end(_path(path), constant.encode(), rows, sizes, len(pools), int(strand), int(mismatches),
                                               int(bool(use_first)), int(bool(diagnostics)), int(nthreads), counts_p, C.byref(total), err, ERRCAP), err)
    return counts[:nch].copy(), int(total.value)


def count_combo_barcodes_paired(path1: str, constant1: str, reverse1: bool, mismatches1: int, pool1: Sequence[str],
                                path2: str, constant2: str, reverse2: bool, mismatches2: int, pool2: Sequence[str],
                                randomized: bool, use_first: bool, nthreads: int = 1):
    """src/count_combo_barcodes_paired.cpp:57-95 -> (indices int32[2, K] 0-based sorted by (first, second),
    freq int32[K], total, barcode1_only, barcode2_only)."""
    L, err = _lib.load(), errbuf()
    total, b1, b2 = C.c_int32(0), C.c_int32(0), C.c_int32(0)
    with combo_outputs(L) as (combos, take):
        check(L.scg_count_combo_barcodes_paired(_path(path1), constant1.encode(), int(bool(reverse1)), int(mismatches1), *_lib.pool(pool1),
                                                _path(path2), constant2.encode(), int(bool(reverse2)), int(mismatches2), *_lib.pool(pool2),
                                                int(bool(randomized)), int(bool(use_first)), int(nthreads), *combos,
                                                C.byref(total), C.byref(b1), C.byref(b2), err, ERRCAP), err)
        idx, freq = take()
    return idx, freq, int(total.value), int(b1.value), int(b2.value)


# =============================================================================================
# Many files in one native call (matrixOf*)
# =============================================================================================
@contextlib.contextmanager
def _devices_env(devices):
    """`devices=` of the matrixOf* mirrors -> scg_set_devices for the duration of one native call on this thread (the C
    ABI's device list; an id may repeat to keep several files in flight on one card).  Nothing touches the process
    environment: libscg's worker threads read it while a call runs."""
    if devices is None:
        yield
        return
    L = _lib.load()
    err = errbuf()
    ids = [int(d) for d in devices]
    arr = (C.c_int * max(len(ids), 1))(*ids)
    check(L.scg_set_devices(arr, len(ids), err, ERRCAP), err)
    try:
        yield
    finally:
        L.scg_set_devices(None, 0, err, ERRCAP)


@contextlib.contextmanager
def _files_call(devices, *path_lists, scalars: int = 1):
    """What the many-files mirrors share around their native call.  `with ... as (n, paths, outs)`: n files; `paths`, one C
    array per list of paths; `outs`, `scalars` caller-allocated int32 arrays of n entries (totals; barcode1_only,
    barcode2_only), read afterwards as `out[:n]`, a list.  Every array has at least one entry, and `devices` is the C ABI's
    device list while the block runs."""
    n = len(path_lists[0])
    paths = [cstr_array([os.fspath(x) for x in p])[0] for p in path_lists]
    outs = [(C.c_int32 * max(n, 1))() for _ in range(scalars)]
    with _devices_env(devices):
        yield n, paths, outs


def _files_counts(n_pool: int, n_files: int):
    """The column-major int32[n_pool, n_files] output of a many-files entry (column f = file f) -> (its pointer for the
    call, take() -> a copy shaped [n_pool, n_files])."""
    buf = np.zeros(max(n_pool * n_files, 1), dtype=np.int32)
    return buf.ctypes.data_as(i32_p), lambda: buf[:n_pool * n_files].reshape(n_files, n_pool).T.copy()


def count_single_barcodes_files(paths: Sequence[str], constant: str, strand: int, pool: Sequence[str], mismatches: int,
                                use_first: bool, nthreads: int = 1, devices=None):
    """scg_count_single_barcodes_files: every file of matrixOfSingleBarcodes in one native call
    -> (counts int32[len(pool), len(paths)], totals list)."""
    L, err = _lib.load(), errbuf()
    counts_p, take_counts = _files_counts(len(pool), len(paths))
    with _files_call(devices, paths) as (n, (farr,), (totals,)):
        check(L.scg_count_single_barcodes_files(farr, n, constant.encode(), int(strand), *_lib.pool(pool), int(mismatches),
                                                int(bool(use_first)), int(nthreads), counts_p, totals, err, ERRCAP), err)
    return take_counts(), totals[:n]


def count_combo_barcodes_single_files(paths: Sequence[str], constant: str, strand: int, pool: Sequence[Sequence[str]], mismatches: int,
                                      use_first: bool, nthreads: int = 1, devices=None):
    """scg_count_combo_barcodes_single_files -> list of (indices int32[2, K], freq int32[K], total), one per file."""
    if len(pool) != 2:
        raise ScgError(_lib.SCG_ERR_INVALID, TWO_REGIONS)
    L, err = _lib.load(), errbuf()
    with _files_call(devices, paths) as (n, (farr,), (totals,)), per_file_combo_outputs(L, n) as (combos, take):
        check(L.scg_count_combo_barcodes_single_files(farr, n, constant.encode(), int(strand), *_lib.pool(pool[0]), *_lib.pool(pool[1]),
                                                      int(mismatches), int(bool(use_first)), int(nthreads), *combos, totals, err, ERRCAP), err)
        return [(idx, freq, total) for (idx, freq), total in zip(take(), totals[:n])]


def count_combo_barcodes_regions_files(paths: Sequence[str], constant: str, strand: int, pools: Sequence[Sequence[str]], mismatches: int,
                                       use_first: bool, nthreads: int = 1, devices=None):
    """scg_count_combo_barcodes_regions_files -> list of (indices int32[len(pools), K], freq int32[K], total), one per file."""
    L, err = _lib.load(), errbuf()
    rows, sizes, _keep = _lib.cstr_matrix(pools)
    with _files_call(devices, paths) as (n, (farr,), (totals,)), per_file_combo_outputs(L, n, max(len(pools), 1)) as (combos, take):
        check(L.scg_count_combo_barcodes_regions_files(farr, n, constant.encode(), int(strand), rows, sizes, len(pools),
                                                       int(mismatches), int(bool(use_first)), int(nthreads), *combos, totals, err, ERRCAP), err)
        return [(idx, freq, total) for (idx, freq), total in zip(take(), totals[:n])]


def count_dual_barcodes_files(paths1: Sequence[str], constant1: str, reverse1: bool, mismatches1: int, pool1: Sequence[str],
                              paths2: Sequence[str], constant2: str, reverse2: bool, mismatches2: int, pool2: Sequence[str],
                              randomized: bool, use_first: bool, nthreads: int = 1, devices=None):
    """scg_count_dual_barcodes_files -> (counts int32[len(pool1), n_files], totals list)."""
    if len(pool1) != len(pool2):
        raise ScgError(_lib.SCG_ERR_INVALID, SAME_LENGTH)
    if len(paths1) != len(paths2):
        raise ValueError("paths1 and paths2 differ in length")
    L, err = _lib.load(), errbuf()
    counts_p, take_counts = _files_counts(len(pool1), len(paths1))
    with _files_call(devices, paths1, paths2) as (n, (f1, f2), (totals,)):
        check(L.scg_count_dual_barcodes_files(f1, constant1.encode(), int(bool(reverse1)), int(mismatches1), cstr_array(pool1)[0],
                                              f2, constant2.encode(), int(bool(reverse2)), int(mismatches2), cstr_array(pool2)[0], len(pool1), n,
                                              int(bool(randomized)), int(bool(use_first)), int(nthreads), counts_p, totals, err, ERRCAP), err)
    return take_counts(), totals[:n]


def count_single_barcodes_paired_files(paths1: Sequence[str], paths2: Sequence[str], constant: str, strand: int, pool: Sequence[str],
                                       mismatches: int, use_first: bool, nthreads: int = 1, devices=None):
    """scg_count_single_barcodes_paired_files -> (counts int32[len(pool), n_files], totals list)."""
    if len(paths1) != len(paths2):
        raise ValueError("paths1 and paths2 differ in length")
    L, err = _lib.load(), errbuf()
    counts_p, take_counts = _files_counts(len(pool), len(paths1))
    with _files_call(devices, paths1, paths2) as (n, (f1, f2), (totals,)):
        check(L.scg_count_single_barcodes_paired_files(f1, f2, n, constant.encode(), int(strand), *_lib.pool(pool), int(mismatches),
                                                       int(bool(use_first)), int(nthreads), counts_p, totals, err, ERRCAP), err)
    return take_counts(), totals[:n]


def count_dual_barcodes_diagnostics_files(paths1: Sequence[str], constant1: str, reverse1: bool, mismatches1: int, pool1: Sequence[str],
                                          paths2: Sequence[str], constant2: str, reverse2: bool, mismatches2: int, pool2: Sequence[str],
                                          randomized: bool, use_first: bool, nthreads: int = 1, devices=None):
    """scg_count_dual_barcodes_diagnostics_files: every pair of files of matrixOfDualBarcodes(include.invalid=TRUE) in one
    native call -> (counts int32[len(pool1), n_files], list of (indices int32[2, K], freq int32[K]) per file, totals list,
    barcode1_only list, barcode2_only list)."""
    if len(pool1) != len(pool2):
        raise ScgError(_lib.SCG_ERR_INVALID, SAME_LENGTH)
    if len(paths1) != len(paths2):
        raise ValueError("paths1 and paths2 differ in length")
    L, err = _lib.load(), errbuf()
    counts_p, take_counts = _files_counts(len(pool1), len(paths1))
    with _files_call(devices, paths1, paths2, scalars=3) as (n, (f1, f2), (totals, b1, b2)), per_file_combo_outputs(L, n) as (combos, take):
        check(L.scg_count_dual_barcodes_diagnostics_files(f1, constant1.encode(), int(bool(reverse1)), int(mismatches1), cstr_array(pool1)[0],
                                                          f2, constant2.encode(), int(bool(reverse2)), int(mismatches2), cstr_array(pool2)[0],
                                                          len(pool1), n, int(bool(randomized)), int(bool(use_first)), int(nthreads),
                                                          counts_p, *combos, totals, b1, b2, err, ERRCAP), err)
        return take_counts(), take(), totals[:n], b1[:n], b2[:n]


def count_dual_barcodes_single_end_files(paths: Sequence[str], constant: str, pools: Sequence[Sequence[str]], strand: int, mismatches: int,
                                         use_first: bool, nthreads: int = 1, devices=None):
    """scg_count_dual_barcodes_single_end_files: every file of matrixOfDualBarcodesSingleEnd in one native call
    -> (counts int32[n combinations, n_files], totals list)."""
    L, err = _lib.load(), errbuf()
    counts_p, take_counts = _files_counts(len(pools[0]) if pools else 0, len(paths))
    rows, sizes, _keep = cstr_matrix(pools)
    with _files_call(devices, paths) as (n, (farr,), (totals,)):
        check(L.scg_count_dual_barcodes_single_end_files(farr, n, constant.encode(), rows, sizes, len(pools), int(strand), int(mismatches),
                                                         int(bool(use_first)), int(nthreads), counts_p, totals, err, ERRCAP), err)
    return take_counts(), totals[:n]


def count_dual_barcodes_single_end_diagnostics_files(paths: Sequence[str], constant: str, pools: Sequence[Sequence[str]], strand: int,
                                                     mismatches: int, use_first: bool, nthreads: int = 1, devices=None):
    """scg_count_dual_barcodes_single_end_diagnostics_files: matrixOfDualBarcodesSingleEnd(include.invalid=TRUE) in one native
    call -> (counts int32[n combinations, n_files], list of (indices int32[2, K], freq int32[K]) per file, totals list)."""
    L, err = _lib.load(), errbuf()
    counts_p, take_counts = _files_counts(len(pools[0]) if pools else 0, len(paths))
    rows, sizes, _keep = cstr_matrix(pools)
    with _files_call(devices, paths) as (n, (farr,), (totals,)), per_file_combo_outputs(L, n) as (combos, take):
        check(L.scg_count_dual_barcodes_single_end_diagnostics_files(farr, n, constant.encode(), rows, sizes, len(pools), int(strand),
                                                                     int(mismatches), int(bool(use_first)), int(nthreads),
                                                                     counts_p, *combos, totals, err, ERRCAP), err)
        return take_counts(), take(), totals[:n]


def count_combo_barcodes_paired_files(paths1: Sequence[str], constant1: str, reverse1: bool, mismatches1: int, pool1: Sequence[str],
                                      paths2: Sequence[str], constant2: str, reverse2: bool, mismatches2: int, pool2: Sequence[str],
                                      randomized: bool, use_first: bool, nthreads: int = 1, devices=None):
    """scg_count_combo_barcodes_paired_files: every pair of files of matrixOfPairedComboBarcodes in one native call
    -> list of (indices int32[2, K], freq int32[K], total, barcode1_only, barcode2_only), one per pair of files."""
    if len(paths1) != len(paths2):
        raise ValueError("paths1 and paths2 differ in length")
    L, err = _lib.load(), errbuf()
    with _files_call(devices, paths1, paths2, scalars=3) as (n, (f1, f2), (totals, b1, b2)), per_file_combo_outputs(L, n) as (combos, take):
        check(L.scg_count_combo_barcodes_paired_files(f1, constant1.encode(), int(bool(reverse1)), int(mismatches1), *_lib.pool(pool1),
                                                      f2, constant2.encode(), int(bool(reverse2)), int(mismatches2), *_lib.pool(pool2), n,
                                                      int(bool(randomized)), int(bool(use_first)), int(nthreads),
                                                      *combos, totals, b1, b2, err, ERRCAP), err)
        return [(idx, freq, *scalars) for (idx, freq), *scalars in zip(take(), totals[:n], b1[:n], b2[:n])]


def count_random_barcodes_files(paths: Sequence[str], constant: str, strand: int, mismatches: int, use_first: bool, nthreads: int = 1,
                                devices=None):
    """scg_count_random_barcodes_files: every file of matrixOfRandomBarcodes in one native call, tallied in HBM
    -> (keys list[str] sorted: the union over the files, matrix int32[K, n_files] dense as R builds it
    (R/countRandomBarcodes.R:87-92), totals int32[n_files])."""
    L, err = _lib.load(), errbuf()
    seq_p, colptr_p, rows_p, freq_p = C.c_void_p(), _lib.i64_p(), i32_p(), i32_p()
    k, vlen = C.c_int64(0), C.c_int32(0)
    with _files_call(devices, paths) as (n, (farr,), (totals,)):
        check(L.scg_count_random_barcodes_files(farr, n, constant.encode(), int(strand), int(mismatches), int(bool(use_first)), int(nthreads),
                                                C.byref(seq_p), C.byref(k), C.byref(vlen), C.byref(colptr_p), C.byref(rows_p), C.byref(freq_p),
                                                totals, err, ERRCAP), err)
    K = int(k.value)
    try:
        keys = _lib.decode_sequences(seq_p, K, int(vlen.value))
        colptr = np.ctypeslib.as_array(colptr_p, shape=(n + 1,)).copy()
        nnz = int(colptr[n])
        rows = np.ctypeslib.as_array(rows_p, shape=(max(nnz, 1),))[:nnz].copy()
        freq = np.ctypeslib.as_array(freq_p, shape=(max(nnz, 1),))[:nnz].copy()
    finally:
        for p in (seq_p, colptr_p, rows_p, freq_p):
            L.scg_free(p)
    matrix = np.zeros((K, n), dtype=np.int32)
    matrix[rows, np.repeat(np.arange(n), np.diff(colptr))] = freq
    return keys, matrix, np.array(totals[:n], dtype=np.int32)


# =============================================================================================
# Combination counts of many files as one matrix (combineComboCounts on the device)
# =============================================================================================
def combine_combinations(lists: Sequence, devices=None):
    """scg_combine_combinations: combineComboCounts (R/combineComboCounts.R:31-57) for per-file lists of
    (indices int32[2, K_f], freq int32[K_f]) in any order -> (indices int32[2, K]: the union sorted by (first, second),
    matrix int32[K, len(lists)] dense)."""
    L, err = _lib.load(), errbuf()
    n = len(lists)
    idx = [np.ascontiguousarray(np.asarray(i, dtype=np.int32).reshape(2, -1).T) for i, _ in lists]     # K_f x 2: the C layout
    freq = [np.ascontiguousarray(f, dtype=np.int32).reshape(-1) for _, f in lists]
    for i, f in zip(idx, freq):
        if len(i) != len(f):
            raise ValueError("indices and freq differ in length")
    idx_p, freq_p, ks = (i32_p * max(n, 1))(), (i32_p * max(n, 1))(), (C.c_int64 * max(n, 1))()
    for f in range(n):
        idx_p[f], freq_p[f], ks[f] = idx[f].ctypes.data_as(i32_p), freq[f].ctypes.data_as(i32_p), len(freq[f])
    with _devices_env(devices), _lib.combo_matrix_outputs(L, n) as (matrix, take):
        check(L.scg_combine_combinations(idx_p, freq_p, ks, n, *matrix, err, ERRCAP), err)
        return take()


def count_combo_barcodes_single_matrix(paths: Sequence[str], constant: str, strand: int, pool: Sequence[Sequence[str]], mismatches: int,
                                       use_first: bool, nthreads: int = 1, devices=None):
    """scg_count_combo_barcodes_single_matrix: matrixOfComboBarcodes in one native call, the files' combinations merged on
    the device -> (indices int32[2, K]: the union sorted by (first, second), matrix int32[K, n_files] dense as
    combineComboCounts builds it, totals int32[n_files])."""
    if len(pool) != 2:
        raise ScgError(_lib.SCG_ERR_INVALID, TWO_REGIONS)
    L, err = _lib.load(), errbuf()
    with _files_call(devices, paths) as (n, (farr,), (totals,)), _lib.combo_matrix_outputs(L, n) as (matrix, take):
        check(L.scg_count_combo_barcodes_single_matrix(farr, n, constant.encode(), int(strand), *_lib.pool(pool[0]), *_lib.pool(pool[1]),
                                                       int(mismatches), int(bool(use_first)), int(nthreads), *matrix, totals, err, ERRCAP), err)
        return (*take(), np.array(totals[:n], dtype=np.int32))


def count_combo_barcodes_paired_matrix(paths1: Sequence[str], constant1: str, reverse1: bool, mismatches1: int, pool1: Sequence[str],
                                       paths2: Sequence[str], constant2: str, reverse2: bool, mismatches2: int, pool2: Sequence[str],
                                       randomized: bool, use_first: bool, nthreads: int = 1, devices=None):
    """scg_count_combo_barcodes_paired_matrix: matrixOfPairedComboBarcodes in one native call -> (indices int32[2, K],
    matrix int32[K, n_files] dense, totals int32[n_files], barcode1_only int32[n_files], barcode2_only int32[n_files])."""
    if len(paths1) != len(paths2):
        raise ValueError("paths1 and paths2 differ in length")
    L, err = _lib.load(), errbuf()
    with _files_call(devices, paths1, paths2, scalars=3) as (n, (f1, f2), (totals, b1, b2)), _lib.combo_matrix_outputs(L, n) as (matrix, take):
        check(L.scg_count_combo_barcodes_paired_matrix(f1, constant1.encode(), int(bool(reverse1)), int(mismatches1), *_lib.pool(pool1),
                                                       f2, constant2.encode(), int(bool(reverse2)), int(mismatches2), *_lib.pool(pool2), n,
                                                       int(bool(randomized)), int(bool(use_first)), int(nthreads),
                                                       *matrix, totals, b1, b2, err, ERRCAP), err)
        return (*take(), *(np.array(x[:n], dtype=np.int32) for x in (totals, b1, b2)))


def combo_compact_device(cells: np.ndarray, n0: int, n1: int):
    """scg_combo_compact_device: engine.combo_compact with the compaction done by the device kernels of the matrix entries
    -> (indices int32[2, K], freq int32[K])."""
    L, err = _lib.load(), errbuf()
    cells = np.ascontiguousarray(cells, dtype=np.int32)
    if cells.size < n0 * n1:
        raise ValueError("cells too short")
    src = cells if cells.size else np.zeros(1, dtype=np.int32)
    with combo_outputs(L) as (combos, take):
        check(L.scg_combo_compact_device(src.ctypes.data_as(i32_p), int(n0), int(n1), *combos, err, ERRCAP), err)
        return take()


# =============================================================================================
# Per-read assignment, match_barcodes, parse_fastq
# =============================================================================================
def assign_single_barcodes(path: str, template: str, strand: int, pool: Sequence[str], mismatches: int = 0, use_first: bool = True,
                           batch_reads: int = 1 << 22, device: int = -1):
    """What every read of a FASTQ file matched: kaori::SimpleSingleMatch::State per read (SimpleSingleMatch.hpp:103-140) as
    an engine.Assignment of five numpy arrays of the file's read count -- index and position int32, mismatches,
    variable_mismatches and reverse int8, -1 everywhere for a read without a match.  The file is parsed on the host
    (parse_fastq) and assigned in batches of batch_reads reads through Plan.assign."""
    from .engine import ASSIGN_FIELDS, Assignment, Plan, upload_reads
    if batch_reads <= 0:
        raise ValueError("batch_reads must be positive")
    seqs, offs = parse_fastq(path)
    n = len(offs) - 1
    parts = [[] for _ in ASSIGN_FIELDS]
    with Plan.single(template, strand, pool, mismatches, use_first, device) as plan:
        for a in range(0, n, batch_reads):
            b = min(n, a + batch_reads)
            lo, hi = int(offs[a]), int(offs[b])
            s, o = upload_reads((seqs[lo:hi], offs[a:b + 1] - offs[a]), "cuda" if device < 0 else f"cuda:{device}")
            for part, t in zip(parts, plan.assign(s, o)):
                part.append(t.cpu().numpy())
    return Assignment(*(np.concatenate(p) if p else np.zeros(0, dtype=np.int32 if f in ("index", "position") else np.int8)
                        for p, f in zip(parts, ASSIGN_FIELDS)))


def match_barcodes(sequences: Sequence[str], choices: Sequence[str], substitutions: int = 0, reverse: bool = False):
    """src/match_barcodes.cpp:6-37 -> (index int32[n] 0-based with -1 for NA, mismatches int32[n] with -1 for NA)."""
    L, err = _lib.load(), errbuf()
    n = len(sequences)
    (idx, idx_p), (mm, mm_p) = _int32_out(n), _int32_out(n)
    check(L.scg_match_barcodes(*_lib.pool(sequences), *_lib.pool(choices), int(substitutions), int(bool(reverse)), idx_p, mm_p, err, ERRCAP), err)
    return idx[:n].copy(), mm[:n].copy()


def parse_fastq(path: str):
    """kaori/FastqReader.hpp:42-110 -> (uint8 sequence bytes, uint64 offsets[n + 1])."""
    L, err = _lib.load(), errbuf()
    seqs_p, offs_p, n = C.c_void_p(), C.c_void_p(), C.c_int64(0)
    check(L.scg_parse_fastq(_path(path), C.byref(seqs_p), C.byref(offs_p), C.byref(n), err, ERRCAP), err)
    try:
        offs = np.ctypeslib.as_array(C.cast(offs_p, C.POINTER(C.c_uint64)), shape=(n.value + 1,)).copy()
        nb = int(offs[-1])
        seqs = np.ctypeslib.as_array(C.cast(seqs_p, C.POINTER(C.c_uint8)), shape=(max(nb, 1),))[:nb].copy()
    finally:
        L.scg_free(seqs_p)
        L.scg_free(offs_p)
    return seqs, offs
