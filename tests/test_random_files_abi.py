"""scg_count_random_barcodes_files (matrixOfRandomBarcodes in one native call) without a GPU: the entry point exists in the
header, the library and the binding; null pointers and a negative file count are refused; every argument check of the
one-file entry is raised, with its code and message, before any device work; no files give an empty matrix."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAME = "scg_count_random_barcodes_files"

BAD_ARGS = [
    ("ACGTACGTAC", 2, 0, "expected one variable region in the constant template"),      # no variable region
    ("ACGT----AC---GT", 2, 0, None),                                                     # two variable regions
    ("ACGT----ACGT", 3, 0, None),                                                        # no such strand
    ("ACGT----ACGT", -1, 0, None),
    ("ACGT----ACGT", 2, -1, "negative number of mismatches"),
]


@pytest.fixture()
def fastq(tmp_path):
    path = tmp_path / "one.fastq"
    path.write_text("@r\nACGTACGTACGT\n+\nIIIIIIIIIIII\n")
    return str(path)


def test_symbol_declared_exported_and_bound(sc):
    from screencounter_amd import _lib
    header = open(os.path.join(ROOT, "include", "scg.h")).read()
    out = subprocess.check_output(["nm", "-D", "--defined-only", _lib.LIB_PATH], text=True)
    exported = {line.split()[-1] for line in out.splitlines() if len(line.split()) >= 3}
    assert f"int {NAME}(" in header
    assert NAME in exported and NAME in _lib.SIGNATURES
    assert hasattr(sc.load(), NAME)
    assert callable(sc.count_random_barcodes_files)


def raw_call(sc, paths, n_files, constant=b"ACGT----ACGT", drop=None, totals=True):
    """The C entry with every output in place, or with the one named by `drop` null -> (return code, message, outputs)."""
    from screencounter_amd import _lib
    L = sc.load()
    out = dict(seq=C.c_void_p(), k=C.c_int64(-1), vlen=C.c_int32(-1), col=_lib.i64_p(), rows=_lib.i32_p(), freq=_lib.i32_p())
    ref = {name: (None if name == drop else C.byref(v)) for name, v in out.items()}
    farr = None
    if paths is not None:
        farr, _keep = _lib.cstr_array(paths)
    tot = (C.c_int32 * 4)() if totals else None
    err = _lib.errbuf()
    rc = L.scg_count_random_barcodes_files(farr, n_files, constant, 2, 0, 1, 1, ref["seq"], ref["k"], ref["vlen"], ref["col"], ref["rows"],
                                           ref["freq"], tot, err, _lib.ERRCAP)
    return rc, err.value.decode(), out


@pytest.mark.parametrize("drop", ["seq", "k", "vlen", "col", "rows", "freq"])
def test_null_outputs(sc, fastq, drop):
    from screencounter_amd import _lib
    for paths, n in (([fastq], 1), ([], 0)):
        rc, _msg, _out = raw_call(sc, paths, n, drop=drop)
        assert rc == _lib.SCG_ERR_INVALID, (drop, n)


def test_null_inputs_and_negative_count(sc, fastq):
    from screencounter_amd import _lib
    INV = _lib.SCG_ERR_INVALID
    assert raw_call(sc, [fastq], -1)[0] == INV
    assert raw_call(sc, None, 1)[0] == INV
    assert raw_call(sc, [fastq], 1, totals=False)[0] == INV
    assert raw_call(sc, [fastq], 1, constant=None)[0] == INV
    L = sc.load()
    farr = (C.c_char_p * 2)(fastq.encode(), None)                        # a null path among the files
    out = dict(seq=C.c_void_p(), k=C.c_int64(-1), vlen=C.c_int32(-1), col=_lib.i64_p(), rows=_lib.i32_p(), freq=_lib.i32_p())
    err = _lib.errbuf()
    rc = L.scg_count_random_barcodes_files(farr, 2, b"ACGT----ACGT", 2, 0, 1, 1, C.byref(out["seq"]), C.byref(out["k"]), C.byref(out["vlen"]),
                                           C.byref(out["col"]), C.byref(out["rows"]), C.byref(out["freq"]), (C.c_int32 * 2)(), err, _lib.ERRCAP)
    assert rc == INV
    assert not out["seq"].value and not out["col"] and not out["rows"] and not out["freq"] and out["k"].value == 0


def outcome(fn):
    from screencounter_amd import _lib
    try:
        return "ok", fn()
    except _lib.ScgError as e:
        return "error", (e.code, str(e))


@pytest.mark.parametrize("template,strand,mismatches,message", BAD_ARGS)
def test_argument_errors_match_the_one_file_entry(sc, fastq, template, strand, mismatches, message):
    """Whatever the one-file entry says to a template, a strand or a budget, the many-files entry says too, with the same
    code and message.  Where the one-file entry has a check (`message`), it is raised with or without a device: the checks
    come first.  (The reference's handler takes a template with two variable regions and uses the first.)"""
    from screencounter_amd import _lib
    one = outcome(lambda: sc.count_random_barcodes(fastq, template, strand, mismatches, True, 1))
    if message is not None:
        assert one[0] == "error" and message in one[1][1] and one[1][0] == _lib.SCG_ERR_INVALID, one
    for paths in ([fastq], [fastq, fastq, fastq]):
        many = outcome(lambda: sc.count_random_barcodes_files(paths, template, strand, mismatches, True, 1))
        assert many[0] == one[0]
        if one[0] == "error":
            assert many[1] == one[1]
            continue
        (seqs, freq), total = one[1]
        keys, matrix, totals = many[1]
        assert keys == seqs and totals.tolist() == [total] * len(paths)
        assert all(matrix[:, c].tolist() == freq.tolist() for c in range(len(paths)))


def test_missing_first_file_comes_before_the_argument_checks(sc, tmp_path):
    """As in a loop over the files: the reader of the first file is opened, then the template is looked at."""
    missing = str(tmp_path / "nope.fastq")
    with pytest.raises(sc.ScgError) as one:
        sc.count_random_barcodes(missing, "ACGTACGTAC", 2, 0, True, 1)
    with pytest.raises(sc.ScgError) as many:
        sc.count_random_barcodes_files([missing, missing], "ACGTACGTAC", 2, 0, True, 1)
    assert (many.value.code, str(many.value)) == (one.value.code, str(one.value))


def test_no_files(sc):
    from screencounter_amd import _lib
    rc, msg, out = raw_call(sc, [], 0)
    assert rc == _lib.SCG_OK, msg
    assert out["k"].value == 0
    assert out["seq"].value and out["col"] and out["rows"] and out["freq"]      # four arrays to release, as after any success
    assert out["col"][0] == 0
    L = sc.load()
    for name in ("seq", "col", "rows", "freq"):
        L.scg_free(out[name])
    rc, msg, out = raw_call(sc, None, 0, totals=False)                          # (nothing to read from, nothing to write to)
    assert rc == _lib.SCG_OK, msg
    for name in ("seq", "col", "rows", "freq"):
        L.scg_free(out[name])
    keys, matrix, totals = sc.count_random_barcodes_files([], "ACGT----ACGT", 2, 0, True, 1)
    assert keys == [] and matrix.shape == (0, 0) and matrix.dtype == np.int32 and totals.shape == (0,)
