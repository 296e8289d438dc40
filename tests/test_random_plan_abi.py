"""Random-barcode plans (scg_plan_random / scg_plan_read_random) without a GPU: the entry points exist, and every argument
check of the file entry point is raised, with its code and message, before any device work."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

NO_REGION = "ACGTACGTAC"
NINE_REGIONS = "AC" + "".join("-A" for _ in range(9)) + "CG"
BAD_ARGS = [
    (NO_REGION, 0, "expected one variable region in the constant template", 1),
    (NINE_REGIONS, 0, "at most 8 variable regions", 4),
    ("ACGT----ACGT", -1, "negative number of mismatches", 1),
]


@pytest.mark.parametrize("template,mismatches,message,code", BAD_ARGS)
def test_plan_random_argument_errors(sc, template, mismatches, message, code):
    with pytest.raises(sc.ScgError, match=message) as ei:
        sc.Plan.random(template, 2, mismatches=mismatches)
    assert ei.value.code == code, (ei.value.code, str(ei.value))


@pytest.mark.parametrize("template,mismatches,message,code", BAD_ARGS)
def test_plan_random_errors_match_file_entry(sc, template, mismatches, message, code, tmp_path):
    fq = tmp_path / "one.fastq"
    fq.write_text("@r\nACGTACGTACGT\n+\nIIIIIIIIIIII\n")
    with pytest.raises(sc.ScgError) as plan_err:
        sc.Plan.random(template, 2, mismatches=mismatches)
    with pytest.raises(sc.ScgError) as file_err:
        sc.count_random_barcodes(str(fq), template, 2, mismatches, True, 1)
    assert (plan_err.value.code, str(plan_err.value)) == (file_err.value.code, str(file_err.value))


def test_plan_random_null_arguments(sc):
    import ctypes as C
    from screencounter_amd import _lib
    L = sc.load()
    err = _lib.errbuf()
    assert L.scg_plan_random(None, b"AC--GT", 0, 0, 1, -1, err, _lib.ERRCAP) == _lib.SCG_ERR_INVALID
    h = C.c_void_p()
    assert L.scg_plan_random(C.byref(h), None, 0, 0, 1, -1, err, _lib.ERRCAP) == _lib.SCG_ERR_INVALID
    assert not h.value
    k, vlen, total = C.c_int64(0), C.c_int32(0), C.c_int64(0)
    seq_p, freq_p = C.c_void_p(), _lib.i32_p()
    assert L.scg_plan_read_random(None, C.byref(seq_p), C.byref(freq_p), C.byref(k), C.byref(vlen), C.byref(total), None,
                                  err, _lib.ERRCAP) == _lib.SCG_ERR_INVALID


def test_plan_random_python_surface(sc):
    assert callable(sc.Plan.random)
    assert callable(getattr(sc.Plan, "read_random"))


def test_random_plan_symbols_declared_and_exported(sc):
    from screencounter_amd import _lib
    header = open(os.path.join(ROOT, "include", "scg.h")).read()
    out = subprocess.check_output(["nm", "-D", "--defined-only", _lib.LIB_PATH], text=True)
    exported = {line.split()[-1] for line in out.splitlines() if len(line.split()) >= 3}
    lib = sc.load()
    for name in ("scg_plan_random", "scg_plan_read_random"):
        assert f"int {name}(" in header
        assert name in exported and name in _lib.SIGNATURES
        assert hasattr(lib, name)
