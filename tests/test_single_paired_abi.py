"""The paired single-barcode handler (kaori::SingleBarcodePairedEnd) without a GPU: its three symbols exist, and their
host-side half behaves as scg_plan_single / scg_count_dual_barcodes / the many-files contract of include/scg.h do --
compile_single's argument errors before any device work, both readers before the arguments in the one-file entry, the
arguments before any file in the many-files entry, null arguments, no files.  What needs a plan (and so a device) is
skipped where there is none."""
import ctypes as C
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ("scg_plan_single_paired", "scg_count_single_barcodes_paired", "scg_count_single_barcodes_paired_files")
TEMPLATE = "ACGT----TGCA"

# (pattern, template, strand, pool): the table test_abi.py::test_plan_argument_checks_precede_device_errors has for Plan.single
BAD_ARGUMENTS = [
    (r"same length \(4\)", TEMPLATE, 2, ["AAAA", "AAA"]),
    (r"duplicate sequences detected \(1, 2\)", TEMPLATE, 2, ["AAAA", "AAAA"]),
    (r"duplicate sequences detected \(1, 3\)", TEMPLATE, 2, ["AAAN", "CCCC", "AAAG"]),
    ("expected one variable region", "ACGT--A--TGCA", 2, ["AAAA"]),
    ("expected one variable region", "ACGTTGCA", 2, ["AAAA"]),
    (r"barcode_pool sequences \(4\) should be the same as the barcode_pool region \(5\)", "ACGT-----TGCA", 2, ["AAAA"]),
    ("unknown base 'X'", "ACXT----TGCA", 0, ["AAAA"]),
    ("cannot complement unknown base 'X'", "ACXT----TGCA", 1, ["AAAA"]),
    ("unknown base 'Z' detected when constructing the trie", TEMPLATE, 2, ["AAZA"]),
    ("longer than 256 bp", "A" * 250 + "----" + "C" * 10, 2, ["AAAA"]),
]


def error_of(sc, fn, *args, **kwargs):
    with pytest.raises(sc.ScgError) as e:
        fn(*args, **kwargs)
    return e.value.code, str(e.value)


def has_device(sc):
    return sc.load().scg_device_count() > 0


@pytest.fixture
def one_read(tmp_path):
    p = tmp_path / "one.fastq"
    p.write_bytes(b"@r\nACGTAAAATGCA\n+\nIIIIIIIIIIII\n")
    return str(p)


def test_symbols_are_declared_exported_and_bound(sc):
    from screencounter_amd import _lib
    header = open(os.path.join(ROOT, "include", "scg.h")).read()
    lib = sc.load()
    for name in SYMBOLS:
        assert re.search(r"\bint " + name + r"\(", header), name
        assert hasattr(lib, name) and name in _lib.SIGNATURES, name
    assert all(hasattr(sc, name) for name in ("count_single_barcodes_paired", "count_single_barcodes_paired_files"))
    assert hasattr(sc.Plan, "single_paired")


@pytest.mark.parametrize("pattern,template,strand,pool", BAD_ARGUMENTS, ids=[f"{i}" for i in range(len(BAD_ARGUMENTS))])
def test_plan_argument_errors_are_compile_singles(sc, tmp_path, one_read, pattern, template, strand, pool):
    """SCG_ERR_INVALID with Plan.single's message, device or no device; the same from the file entries -- the one-file entry
    on files that exist, the many-files entry on files that do not (it looks at its arguments first)."""
    from screencounter_amd import _lib
    got = error_of(sc, sc.Plan.single_paired, template, strand, pool)
    assert got[0] == _lib.SCG_ERR_INVALID and re.search(pattern, got[1]), got
    assert got == error_of(sc, sc.Plan.single, template, strand, pool)
    assert got == error_of(sc, sc.count_single_barcodes_paired, one_read, one_read, template, strand, pool, 0, True)
    nowhere = [str(tmp_path / f"nowhere{i}.fastq") for i in range(2)]
    assert got == error_of(sc, sc.count_single_barcodes_paired_files, nowhere, nowhere, template, strand, pool, 0, True)


def test_negative_mismatches(sc):
    from screencounter_amd import _lib
    assert error_of(sc, sc.Plan.single_paired, TEMPLATE, 2, ["AAAA"], -1) == (_lib.SCG_ERR_INVALID, "negative number of mismatches")


def test_valid_plan_needs_a_device_or_works(sc):
    from screencounter_amd import _lib
    if has_device(sc):
        with sc.Plan.single_paired(TEMPLATE, 2, ["AAAA", "CCCC"], 1, False) as p:
            assert p.num_counters == 2 and p.kind == "single_paired"
    else:
        code, msg = error_of(sc, sc.Plan.single_paired, TEMPLATE, 2, ["AAAA", "CCCC"], 1, False)
        assert code == _lib.SCG_ERR_DEVICE and "no HIP device" in msg


def test_missing_files_come_before_a_bad_pool(sc, tmp_path, one_read):
    """Both readers are opened before the arguments are looked at, as in scg_count_dual_barcodes."""
    from screencounter_amd import _lib
    nope = str(tmp_path / "nope.fastq")
    bad_pool = ["AAAA", "AAA"]
    for p1, p2 in ((nope, one_read), (one_read, nope), (nope, nope)):
        code, msg = error_of(sc, sc.count_single_barcodes_paired, p1, p2, TEMPLATE, 2, bad_pool, 0, True)
        assert code == _lib.SCG_ERR_IO and "failed to open file" in msg, (code, msg)
    code, msg = error_of(sc, sc.count_single_barcodes_paired, one_read, one_read, TEMPLATE, 2, bad_pool, 0, True)
    assert code == _lib.SCG_ERR_INVALID and "same length" in msg


def test_valid_file_arguments_need_a_device(sc, tmp_path, one_read):
    from screencounter_amd import _lib
    nowhere = [str(tmp_path / f"nowhere{i}.fastq") for i in range(2)]
    code, msg = error_of(sc, sc.count_single_barcodes_paired_files, nowhere, nowhere, TEMPLATE, 2, ["AAAA", "CCCC"], 0, True)
    if has_device(sc):
        assert code == _lib.SCG_ERR_IO and "nowhere0.fastq" in msg, (code, msg)
    else:
        assert code == _lib.SCG_ERR_DEVICE and "no HIP device" in msg, (code, msg)
        code, msg = error_of(sc, sc.count_single_barcodes_paired, one_read, one_read, TEMPLATE, 2, ["AAAA", "CCCC"], 0, True)
        assert code == _lib.SCG_ERR_DEVICE and "no HIP device" in msg, (code, msg)


def test_no_files(sc):
    counts, totals = sc.count_single_barcodes_paired_files([], [], TEMPLATE, 2, ["AAAA", "CCCC"], 0, True)
    assert counts.shape == (2, 0) and totals == []
    with pytest.raises(ValueError):
        sc.count_single_barcodes_paired_files(["a"], [], TEMPLATE, 2, ["AAAA"], 0, True)


class Raw:
    """Argument lists of the two file entries with every pointer in place; `without` nulls one of them by name."""

    def __init__(self, tmp_path):
        from screencounter_amd import _lib
        self.lib, self.L = _lib, _lib.load()
        self.paths1, self._k1 = _lib.cstr_array([str(tmp_path / f"a{i}.fastq") for i in range(2)])
        self.paths2, self._k2 = _lib.cstr_array([str(tmp_path / f"b{i}.fastq") for i in range(2)])
        self.path1, self.path2 = str(tmp_path / "a0.fastq").encode(), str(tmp_path / "b0.fastq").encode()
        self.pool, self._k3 = _lib.cstr_array(["AAAA", "CCCC"])
        self.counts, self.totals = (C.c_int32 * 4)(), (C.c_int32 * 2)()
        self.err = _lib.errbuf()

    def files(self, without=None, n_files=2):
        a = {n: (None if n == without else getattr(self, n)) for n in ("paths1", "paths2", "counts", "totals")}
        rc = self.L.scg_count_single_barcodes_paired_files(a["paths1"], a["paths2"], n_files, TEMPLATE.encode(), 2, self.pool, 2, 0, 1, 1,
                                                           a["counts"], a["totals"], self.err, self.lib.ERRCAP)
        return rc, self.err.value.decode()

    def one(self, without=None):
        a = {n: (None if n == without else getattr(self, n)) for n in ("path1", "path2", "counts", "totals")}
        rc = self.L.scg_count_single_barcodes_paired(a["path1"], a["path2"], TEMPLATE.encode(), 2, self.pool, 2, 0, 1, 1,
                                                     a["counts"], a["totals"], self.err, self.lib.ERRCAP)
        return rc, self.err.value.decode()


def test_null_arguments(sc, tmp_path):
    from screencounter_amd import _lib
    null = (_lib.SCG_ERR_INVALID, "null argument")
    raw = Raw(tmp_path)
    for name in ("path1", "path2", "counts", "totals"):
        assert raw.one(without=name) == null, name
    for name in ("paths1", "paths2", "counts", "totals"):
        assert raw.files(without=name) == null, name
    assert raw.files(n_files=-1) == null
    raw.paths2[1] = None                                   # a null entry inside a list of paths
    assert raw.files() == null
    raw.totals[0] = 77                                     # no files: nothing is needed, nothing is written
    for name in (None, "paths1", "paths2", "counts", "totals"):
        assert raw.files(without=name, n_files=0) == (_lib.SCG_OK, ""), name
    assert raw.totals[0] == 77
    # the plan entry
    h, err = C.c_void_p(), _lib.errbuf()
    L = _lib.load()
    assert L.scg_plan_single_paired(None, TEMPLATE.encode(), 2, raw.pool, 2, 0, 1, -1, err, _lib.ERRCAP) == _lib.SCG_ERR_INVALID
    assert L.scg_plan_single_paired(C.byref(h), None, 2, raw.pool, 2, 0, 1, -1, err, _lib.ERRCAP) == _lib.SCG_ERR_INVALID
    assert err.value == b"null argument"
    assert L.scg_plan_single_paired(C.byref(h), TEMPLATE.encode(), 2, None, 2, 0, 1, -1, err, _lib.ERRCAP) == _lib.SCG_ERR_INVALID
    assert err.value == b"null argument" and not h.value


def test_batches_go_through_the_paired_entry_only(sc):
    """scg_count_batch refuses the new plan and names the entry to use; scg_count_batch_paired still refuses a single plan.
    The refusals come before the read arguments are looked at, so null batches do."""
    from screencounter_amd import _lib
    if not has_device(sc):
        pytest.skip("a plan needs a device")
    L = sc.load()
    err = _lib.errbuf()
    with sc.Plan.single_paired(TEMPLATE, 2, ["AAAA", "CCCC"]) as p:
        assert L.scg_count_batch(p._h, None, None, 12, 12, 1, None, err, _lib.ERRCAP) == _lib.SCG_ERR_INVALID
        assert b"scg_count_batch_paired" in err.value
    with sc.Plan.single(TEMPLATE, 2, ["AAAA", "CCCC"]) as p:
        assert L.scg_count_batch_paired(p._h, None, None, 12, None, None, 12, 12, 1, None, err, _lib.ERRCAP) == _lib.SCG_ERR_INVALID
        assert err.value == b"scg_count_batch_paired needs a dual plan"
