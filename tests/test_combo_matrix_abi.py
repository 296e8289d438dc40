"""The combination-matrix entries of include/scg.h without a GPU -- scg_combine_combinations,
scg_count_combo_barcodes_single_matrix, scg_count_combo_barcodes_paired_matrix and scg_combo_compact_device: the symbols
are declared, exported and bound; null pointers and a negative file count are refused; a missing first file and the
argument errors carry the one-file entries' messages and come before any device work; after any failure the four
out-pointers are null and K is 0; no files give an empty matrix with four arrays to release; and a valid call without a
device is SCG_ERR_DEVICE.  Every expectation is stated for a machine with and without a device."""
import ctypes as C
import os
import shutil
import subprocess

import numpy as np
import pytest

from tests import combo_matrix_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ["scg_combine_combinations", "scg_count_combo_barcodes_single_matrix", "scg_count_combo_barcodes_paired_matrix",
         "scg_combo_compact_device"]
COMBO, MATE1, MATE2 = "ACGT----TG--CA", "AC--GT", "TT---A"
POOL4, POOL2, POOL3 = ["AAAA", "CCCC"], ["CC", "GG"], ["AAA", "TTT"]
RECORD = b"@r\nACGTAAAATGCCCA\n+\nIIIIIIIIIIIIII\n"


def has_device(sc):
    return sc.load().scg_device_count() > 0


def error_of(sc, fn, *args):
    with pytest.raises(sc.ScgError) as e:
        fn(*args)
    return e.value.code, str(e.value)


@pytest.fixture()
def fastq(tmp_path):
    path = tmp_path / "one.fastq"
    path.write_bytes(RECORD)
    return str(path)


class Matrix:
    """The five outputs of a matrix entry, holding what an uninitialised caller may hold."""

    def __init__(self):
        from screencounter_amd import _lib
        self.junk = (C.c_int32 * 2)()
        self.idx, self.rows, self.freq = (C.cast(self.junk, _lib.i32_p) for _ in range(3))
        self.col = C.cast(self.junk, _lib.i64_p)
        self.k = C.c_int64(5)

    def refs(self, drop=None):
        named = dict(idx=self.idx, k=self.k, col=self.col, rows=self.rows, freq=self.freq)
        return [None if name == drop else C.byref(v) for name, v in named.items()]

    def all_null(self):
        return not self.idx and not self.col and not self.rows and not self.freq and self.k.value == 0

    def release(self, L):
        assert self.idx and self.col and self.rows and self.freq
        for p in (self.idx, self.col, self.rows, self.freq):
            L.scg_free(p)


def path_array(paths):
    """A C array of paths in which an entry may be null, or a null pointer for None."""
    if paths is None:
        return None
    return (C.c_char_p * max(len(paths), 1))(*[None if p is None else p.encode() for p in paths])


def raw_single(sc, paths, n_files, out, drop=None, totals=True, template=COMBO):
    from screencounter_amd import _lib
    farr = path_array(paths)
    p0, p1 = _lib.cstr_array(POOL4)[0], _lib.cstr_array(POOL2)[0]
    err = _lib.errbuf()
    rc = sc.load().scg_count_combo_barcodes_single_matrix(farr, n_files, template.encode(), 2, p0, 2, p1, 2, 0, 1, 1, *out.refs(drop),
                                                          (C.c_int32 * 4)() if totals else None, err, _lib.ERRCAP)
    return rc, err.value.decode()


def raw_paired(sc, paths1, paths2, n_files, out, drop=None, scalars=(True, True, True), template=MATE1):
    from screencounter_amd import _lib
    f1, f2 = path_array(paths1), path_array(paths2)
    p1, p2 = _lib.cstr_array(POOL2)[0], _lib.cstr_array(POOL3)[0]
    err = _lib.errbuf()
    tot, b1, b2 = ((C.c_int32 * 4)() if s else None for s in scalars)
    rc = sc.load().scg_count_combo_barcodes_paired_matrix(f1, template.encode(), 0, 0, p1, 2, f2, MATE2.encode(), 0, 0, p2, 2, n_files, 0, 1, 1,
                                                          *out.refs(drop), tot, b1, b2, err, _lib.ERRCAP)
    return rc, err.value.decode()


def raw_combine(sc, lists, n_files, out, drop=None, null=None):
    """lists: per file (K_f x 2 pairs, counts); `null`: "indices", "freq" or "k" passes that argument as a null pointer."""
    from screencounter_amd import _lib
    n = max(len(lists), 1)
    idx, freq, ks = (_lib.i32_p * n)(), (_lib.i32_p * n)(), (C.c_int64 * n)()
    keep = []
    for f, (pairs, counts) in enumerate(lists):
        a, b = np.ascontiguousarray(pairs, dtype=np.int32).reshape(-1), np.ascontiguousarray(counts, dtype=np.int32)
        keep += [a, b]
        idx[f], freq[f], ks[f] = a.ctypes.data_as(_lib.i32_p), b.ctypes.data_as(_lib.i32_p), len(b)
    err = _lib.errbuf()
    rc = sc.load().scg_combine_combinations(None if null == "indices" else idx, None if null == "freq" else freq, None if null == "k" else ks,
                                            n_files, *out.refs(drop), err, _lib.ERRCAP)
    return rc, err.value.decode()


# ---- the symbols ------------------------------------------------------------------------------------------------------
def test_symbols_declared_exported_and_bound(sc):
    from screencounter_amd import _lib
    header = open(os.path.join(ROOT, "include", "scg.h")).read()
    out = subprocess.check_output(["nm", "-D", "--defined-only", _lib.LIB_PATH], text=True)
    exported = {line.split()[-1] for line in out.splitlines() if len(line.split()) >= 3}
    for name in NAMES:
        assert f"int {name}(" in header, name
        assert name in exported and name in _lib.SIGNATURES, name
        assert getattr(sc.load(), name).argtypes == _lib.SIGNATURES[name][1]
    for mirror in ("combine_combinations", "count_combo_barcodes_single_matrix", "count_combo_barcodes_paired_matrix", "combo_compact_device"):
        assert callable(getattr(sc, mirror)), mirror


def test_the_tile_size_is_a_named_constant_of_the_launch_header():
    tile = ref.tile_cells()
    assert tile >= 1024 and tile % 1024 == 0            # 256 lanes x 16-byte loads of int32 cells


@pytest.mark.skipif(shutil.which("g++") is None, reason="no g++")
def test_shim_type_checks_and_binds_the_three_entries():
    shim = os.path.join(ROOT, "shim", "scg_shim.cpp")
    subprocess.check_call(["g++", "-std=c++17", "-fsyntax-only", "-Wall", "-Wextra", "-Werror",
                           "-I" + os.path.join(ROOT, "tests", "fake_rcpp"), "-I" + os.path.join(ROOT, "include"), shim])
    text = open(shim).read()
    for name in NAMES[:3]:
        assert name + "(" in text, name


# ---- null pointers, a negative file count -----------------------------------------------------------------------------
@pytest.mark.parametrize("drop", ["idx", "k", "col", "rows", "freq"])
def test_null_outputs(sc, fastq, drop):
    from screencounter_amd import _lib
    null = (_lib.SCG_ERR_INVALID, "null argument")
    for n in (1, 0):
        paths = [fastq] * n
        assert raw_single(sc, paths, n, Matrix(), drop=drop) == null
        assert raw_paired(sc, paths, paths, n, Matrix(), drop=drop) == null
        assert raw_combine(sc, [([[0, 0]], [1])] * n, n, Matrix(), drop=drop) == null


def test_null_inputs_and_negative_count(sc, fastq):
    from screencounter_amd import _lib
    null = (_lib.SCG_ERR_INVALID, "null argument")
    calls = [
        lambda o: raw_single(sc, [fastq], -1, o),
        lambda o: raw_single(sc, None, 1, o),
        lambda o: raw_single(sc, [fastq], 1, o, totals=False),
        lambda o: raw_single(sc, [fastq, None], 2, o),
        lambda o: raw_paired(sc, [fastq], [fastq], -1, o),
        lambda o: raw_paired(sc, None, [fastq], 1, o),
        lambda o: raw_paired(sc, [fastq], None, 1, o),
        lambda o: raw_paired(sc, [fastq, fastq], [fastq, None], 2, o),
        lambda o: raw_paired(sc, [fastq], [fastq], 1, o, scalars=(False, True, True)),
        lambda o: raw_paired(sc, [fastq], [fastq], 1, o, scalars=(True, False, True)),
        lambda o: raw_paired(sc, [fastq], [fastq], 1, o, scalars=(True, True, False)),
        lambda o: raw_combine(sc, [([[0, 0]], [1])], -1, o),
        lambda o: raw_combine(sc, [([[0, 0]], [1])], 1, o, null="indices"),
        lambda o: raw_combine(sc, [([[0, 0]], [1])], 1, o, null="freq"),
        lambda o: raw_combine(sc, [([[0, 0]], [1])], 1, o, null="k"),
    ]
    for i, call in enumerate(calls):
        out = Matrix()
        assert call(out) == null, i
        assert out.all_null(), i


def test_compact_device_null_arguments(sc):
    from screencounter_amd import _lib
    L = sc.load()
    cells = (C.c_int32 * 4)(0, 1, 0, 2)
    for drop in range(4):
        idx, freq, k = _lib.i32_p(), _lib.i32_p(), C.c_int64(5)
        args = [cells, C.byref(idx), C.byref(freq), C.byref(k)]
        args[drop] = None
        err = _lib.errbuf()
        rc = L.scg_combo_compact_device(args[0], 2, 2, args[1], args[2], args[3], err, _lib.ERRCAP)
        assert (rc, err.value.decode()) == (_lib.SCG_ERR_INVALID, "null argument")
        assert not idx and not freq


# ---- the order of the errors ------------------------------------------------------------------------------------------
BAD_SINGLE = [dict(template="ACGT----TGCA"), dict(pool=(["AAAA", "AAAA"], POOL2)), dict(pool=(["AAAA", "AAA"], POOL2)), dict(mismatches=-1)]


@pytest.mark.parametrize("wrong", BAD_SINGLE, ids=["one region", "duplicated barcode", "ragged pool", "negative budget"])
def test_single_matrix_errors_are_the_one_file_entrys_and_come_before_the_device(sc, tmp_path, fastq, wrong):
    """The reader of file 0 first, then the handler's checks, then the device: the same outcome with and without one."""
    from screencounter_amd import _lib
    missing = str(tmp_path / "nope.fastq")

    def args(paths, template=COMBO, pool=(POOL4, POOL2), mismatches=0):
        return paths, template, 2, list(pool), mismatches, True, 1

    for kwargs in ({}, wrong):                              # a missing first file, whatever else is wrong
        one = error_of(sc, sc.count_combo_barcodes_single, *args(missing, **kwargs))
        assert one[0] == _lib.SCG_ERR_IO and "nope.fastq" in one[1]
        assert error_of(sc, sc.count_combo_barcodes_single_matrix, *args([missing, fastq], **kwargs)) == one
    # file 0 is there: the argument error, with the one-file entry's words where that entry gets as far without a device
    # file 0 is there: the argument error, in the one-file entry's words
    many = error_of(sc, sc.count_combo_barcodes_single_matrix, *args([fastq, missing], **wrong))
    assert many[0] == _lib.SCG_ERR_INVALID, many
    assert many == error_of(sc, sc.count_combo_barcodes_single, *args(fastq, **wrong))
    out = Matrix()
    rc, _msg = raw_single(sc, [fastq, missing], 2, out, template="ACGT----TGCA")
    assert rc == _lib.SCG_ERR_INVALID and out.all_null()


@pytest.mark.parametrize("wrong", [dict(template="AC--G-T"), dict(pool1=["AA", "CCC"]), dict(mismatches=-1)], ids=["two regions", "ragged pool", "negative budget"])
def test_paired_matrix_argument_errors_come_before_files_and_device(sc, tmp_path, wrong):
    """As scg_count_combo_barcodes_paired_files: the arguments are looked at before any file is opened."""
    from screencounter_amd import _lib
    a, b = [str(tmp_path / f"a{i}.fastq") for i in range(2)], [str(tmp_path / f"b{i}.fastq") for i in range(2)]

    def args(template=MATE1, pool1=POOL2, mismatches=0):
        return a, template, False, mismatches, pool1, b, MATE2, False, 0, POOL3, False, True, 1

    files = error_of(sc, sc.count_combo_barcodes_paired_files, *args(**wrong))
    assert files[0] == _lib.SCG_ERR_INVALID, files
    assert error_of(sc, sc.count_combo_barcodes_paired_matrix, *args(**wrong)) == files
    out = Matrix()
    rc, _msg = raw_paired(sc, a, b, 2, out, template="AC--G-T")
    assert rc == _lib.SCG_ERR_INVALID and out.all_null()


def test_paired_matrix_missing_file(sc, tmp_path):
    """Valid arguments and no files on disk: with a device the first pair's reader fails; without one the device list does."""
    from screencounter_amd import _lib
    a, b = [str(tmp_path / "a0.fastq")], [str(tmp_path / "b0.fastq")]
    code, msg = error_of(sc, sc.count_combo_barcodes_paired_matrix, a, MATE1, False, 0, POOL2, b, MATE2, False, 0, POOL3, False, True, 1)
    if has_device(sc):
        assert code == _lib.SCG_ERR_IO and "a0.fastq" in msg
    else:
        assert code == _lib.SCG_ERR_DEVICE and "no HIP device" in msg


def test_combine_argument_errors(sc):
    from screencounter_amd import _lib
    for lists in ([([[0, 1], [-1, 2]], [1, 1])], [([[0, 1]], [1]), ([[3, -7]], [2])]):
        out = Matrix()
        rc, msg = raw_combine(sc, lists, len(lists), out)
        assert rc == _lib.SCG_ERR_INVALID and "negative" in msg and out.all_null()


# ---- no files; no device ----------------------------------------------------------------------------------------------
def test_no_files(sc):
    from screencounter_amd import _lib
    L = sc.load()
    for call in (lambda o: raw_single(sc, [], 0, o), lambda o: raw_single(sc, None, 0, o, totals=False),
                 lambda o: raw_paired(sc, [], [], 0, o), lambda o: raw_paired(sc, None, None, 0, o, scalars=(False, False, False)),
                 lambda o: raw_combine(sc, [], 0, o), lambda o: raw_combine(sc, [], 0, o, null="indices")):
        out = Matrix()
        assert call(out) == (_lib.SCG_OK, "")
        assert out.k.value == 0 and out.col[0] == 0
        out.release(L)
    idx, matrix, totals = sc.count_combo_barcodes_single_matrix([], COMBO, 2, [POOL4, POOL2], 0, True, 1)
    assert idx.shape == (2, 0) and matrix.shape == (0, 0) and matrix.dtype == np.int32 and totals.shape == (0,)
    idx, matrix, totals, b1, b2 = sc.count_combo_barcodes_paired_matrix([], MATE1, False, 0, POOL2, [], MATE2, False, 0, POOL3, False, True, 1)
    assert idx.shape == (2, 0) and matrix.shape == (0, 0) and totals.shape == b1.shape == b2.shape == (0,)
    ref.assert_matrix(sc.combine_combinations([]), ref.combine([]))


def test_a_valid_call_needs_a_device(sc, fastq):
    """Without a device every valid call with something to do is SCG_ERR_DEVICE; with one, these small calls succeed."""
    from screencounter_amd import _lib
    for fn, args in ((sc.count_combo_barcodes_single_matrix, ([fastq, fastq], COMBO, 2, [POOL4, POOL2], 0, True, 1)),
                     (sc.count_combo_barcodes_paired_matrix, ([fastq], MATE1, False, 0, POOL2, [fastq], MATE2, False, 0, POOL3, False, True, 1)),
                     (sc.combine_combinations, ([(np.array([[0], [1]]), np.array([3]))],)),
                     (sc.combine_combinations, ([(np.zeros((2, 0)), np.zeros(0))],)),
                     (sc.combo_compact_device, (np.array([0, 1, 0, 2], dtype=np.int32), 2, 2))):
        if has_device(sc):
            fn(*args)
            continue
        code, msg = error_of(sc, fn, *args)
        assert code == _lib.SCG_ERR_DEVICE and "no HIP device" in msg, (fn.__name__, code, msg)
