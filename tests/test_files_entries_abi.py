"""The many-files entries of the dual-diagnostics, single-end dual and paired-combination handlers, without a GPU: the
symbols exist, and their host-side half behaves as the contract above "Many files in one call" (include/scg.h) says --
the argument errors of the single-file sibling, with its code and message, before any file is opened or any device is
touched; null arguments; no files; and, with valid arguments, a loud SCG_ERR_DEVICE where there is no device.

The paths of every call here do not exist, so a call that opened a file before it checked its arguments would report
SCG_ERR_IO."""
import ctypes as C
import re

import pytest

TEMPLATE1, TEMPLATE2 = "AC--GT", "AC--GT"
SE_TEMPLATE = "ACGT----TG--CA"
NINE = "AC" + "--GT" * 9
THREE = "AC--GT--GT--GT"


def missing(tmp_path, n=2, stem="nowhere"):
    return [str(tmp_path / f"{stem}{i}.fastq") for i in range(n)]


@pytest.fixture
def one_read(tmp_path):
    """A file that exists, for the single-file siblings (they open their reader before they look at the arguments)."""
    p = tmp_path / "one.fastq"
    p.write_bytes(b"@r\nACGTAAAATGCCCA\n+\nIIIIIIIIIIIIII\n")
    return str(p)


# (entry, arguments between the paths and the trailing options) -> the calls of the many-files entry and of its sibling
def dual_diag(sc, paths, one, t1, pool1, t2, pool2):
    if paths is None:
        return sc.count_dual_barcodes(one, t1, False, 0, pool1, one, t2, False, 0, pool2, False, True, True, 1)
    return sc.count_dual_barcodes_diagnostics_files(paths, t1, False, 0, pool1, paths, t2, False, 0, pool2, False, True, 1)


def combo_paired(sc, paths, one, t1, pool1, t2, pool2):
    if paths is None:
        return sc.count_combo_barcodes_paired(one, t1, False, 0, pool1, one, t2, False, 0, pool2, False, True, 1)
    return sc.count_combo_barcodes_paired_files(paths, t1, False, 0, pool1, paths, t2, False, 0, pool2, False, True, 1)


def single_end(sc, paths, one, template, pools):
    if paths is None:
        return sc.count_dual_barcodes_single_end(one, template, pools, 2, 0, True, False, 1)
    return sc.count_dual_barcodes_single_end_files(paths, template, pools, 2, 0, True, 1)


def single_end_diag(sc, paths, one, template, pools):
    if paths is None:
        return sc.count_dual_barcodes_single_end(one, template, pools, 2, 0, True, True, 1)
    return sc.count_dual_barcodes_single_end_diagnostics_files(paths, template, pools, 2, 0, True, 1)


def inv():
    from screencounter_amd import _lib
    return _lib.SCG_ERR_INVALID


def uns():
    from screencounter_amd import _lib
    return _lib.SCG_ERR_UNSUPPORTED


PAIRED_DUAL_CASES = [
    # the cases of scg_plan_dual in test_abi.py::test_plan_argument_checks_precede_device_errors
    ("pools differ in length", inv, "both barcode pools should be of the same length", (TEMPLATE1, ["AA", "CC"], TEMPLATE2, ["AA"])),
    ("two regions in template 2", inv, "expected one variable region in the second constant template", (TEMPLATE1, ["AA"], "AC--G-T", ["AA"])),
    ("duplicate pairs", inv, r"duplicate sequences detected \(1, 2\)", (TEMPLATE1, ["AA", "AA"], TEMPLATE2, ["CC", "CC"])),
    ("pool / region length", inv, r"length of variable sequences \(3\) should be the same as the variable region \(2\)",
     (TEMPLATE1, ["AAA"], TEMPLATE2, ["CC"])),
    ("barcodes differ in length", inv, r"same length \(2\)", (TEMPLATE1, ["AA", "CCC"], TEMPLATE2, ["CC", "GG"])),
]
PAIRED_COMBO_CASES = [
    ("no region in template 1", inv, "expected one variable region in the constant template", ("ACGT", ["AA"], TEMPLATE2, ["AA"])),
    ("two regions in template 2", inv, "expected one variable region in the constant template", (TEMPLATE1, ["AA"], "AC--G-T", ["AA"])),
    ("duplicates in a pool", inv, r"duplicate sequences detected \(1, 2\)", (TEMPLATE1, ["AA", "AA"], TEMPLATE2, ["CC", "GG"])),
    ("pool / region length", inv, r"length of barcode_pool sequences \(3\) should be the same as the barcode_pool region \(2\)",
     (TEMPLATE1, ["AAA"], TEMPLATE2, ["CC"])),
    ("barcodes differ in length", inv, r"same length \(2\)", (TEMPLATE1, ["AA", "CC"], TEMPLATE2, ["CC", "GGG"])),
]
SINGLE_END_CASES = [
    # the cases of scg_plan_dual_single_end there
    ("wrong region count", inv, "length of 'barcode_pools' should equal the number of variable regions", (SE_TEMPLATE, [["AAAA"]])),
    ("pool / region length", inv, r"length of variable region 2 \(2\) should be the same as its sequences \(3\)", (SE_TEMPLATE, [["AAAA"], ["CCC"]])),
    ("pools differ in length", inv, "all entries of 'barcode_pools' should have the same length", (SE_TEMPLATE, [["AAAA", "CCCC"], ["CC"]])),
    ("duplicate pairs", inv, r"duplicate sequences detected \(1, 2\)", (SE_TEMPLATE, [["AAAA", "AAAA"], ["CC", "CC"]])),
    ("nine regions", uns, r"1 to 8 variable regions \(got 9\)", (NINE, [["AA"]] * 9)),
]
SINGLE_END_DIAG_CASES = SINGLE_END_CASES + [
    ("diagnostics with three regions", inv, "expected 2 variable regions in the constant template", (THREE, [["AA"], ["CC"], ["GG"]])),
]
ENTRIES = [(dual_diag, PAIRED_DUAL_CASES), (combo_paired, PAIRED_COMBO_CASES), (single_end, SINGLE_END_CASES),
           (single_end_diag, SINGLE_END_DIAG_CASES)]
ARGUMENT_CASES = [pytest.param(fn, code, pattern, args, id=f"{fn.__name__}:{name}")
                  for fn, cases in ENTRIES for name, code, pattern, args in cases]


def error_of(sc, fn, *args):
    with pytest.raises(sc.ScgError) as e:
        fn(sc, *args)
    return e.value.code, str(e.value)


@pytest.mark.parametrize("fn,code,pattern,args", ARGUMENT_CASES)
def test_argument_errors_are_the_single_file_entrys(sc, tmp_path, one_read, fn, code, pattern, args):
    got = error_of(sc, fn, missing(tmp_path), one_read, *args)
    assert got[0] == code() and re.search(pattern, got[1]), got
    assert got == error_of(sc, fn, None, one_read, *args)       # the sibling on a file that exists: same code, same message


VALID = [(dual_diag, (TEMPLATE1, ["AA", "CC"], TEMPLATE2, ["CC", "GG"])),
         (combo_paired, (TEMPLATE1, ["AA", "CC"], TEMPLATE2, ["CC", "GG", "TT"])),
         (single_end, (SE_TEMPLATE, [["AAAA", "CCCC"], ["CC", "GG"]])),
         (single_end_diag, (SE_TEMPLATE, [["AAAA", "CCCC"], ["CC", "GG"]]))]


@pytest.mark.parametrize("fn,args", VALID, ids=[fn.__name__ for fn, _ in VALID])
def test_valid_arguments_need_a_device(sc, tmp_path, one_read, fn, args):
    """No CPU fall-back: without a device SCG_ERR_DEVICE, whatever the files are; with one, the missing first file."""
    from screencounter_amd import _lib
    code, msg = error_of(sc, fn, missing(tmp_path), one_read, *args)
    if sc.load().scg_device_count() == 0:
        assert code == _lib.SCG_ERR_DEVICE and "no HIP device" in msg, (code, msg)
    else:
        assert code == _lib.SCG_ERR_IO and "nowhere0.fastq" in msg, (code, msg)


@pytest.mark.parametrize("fn,args", VALID, ids=[fn.__name__ for fn, _ in VALID])
def test_no_files(sc, fn, args):
    """n_files == 0 succeeds and touches nothing, device or no device, like scg_count_single_barcodes_files."""
    out = fn(sc, [], None, *args)
    if fn is combo_paired:
        assert out == []
        return
    n_pool = len(args[1]) if fn is dual_diag else len(args[1][0])
    assert out[0].shape == (n_pool, 0) and all(part == [] for part in out[1:]), out


# ---- the raw symbols: null arguments -----------------------------------------------------------------------------------
class Raw:
    """Argument lists for the four symbols with every pointer in place; `without` nulls one of them by name."""

    def __init__(self, tmp_path):
        from screencounter_amd import _lib
        self.lib = _lib
        self.L = _lib.load()
        self.n = 2
        self.paths, self._k0 = _lib.cstr_array(missing(tmp_path))
        self.pool1, self._k1 = _lib.cstr_array(["AA", "CC"])
        self.pool2, self._k2 = _lib.cstr_array(["CC", "GG"])
        self.rows, self.sizes, self._k3 = _lib.cstr_matrix([["AAAA", "CCCC"], ["CC", "GG"]])
        self.counts = (C.c_int32 * 8)()
        self.idx, self.freq = (_lib.i32_p * 2)(), (_lib.i32_p * 2)()
        self.k = (C.c_int64 * 2)()
        self.totals, self.b1, self.b2 = (C.c_int32 * 2)(), (C.c_int32 * 2)(), (C.c_int32 * 2)()
        self.err = _lib.errbuf()

    def call(self, symbol, without=None, n_files=None):
        a = {name: (None if name == without else getattr(self, name))
             for name in ("paths", "counts", "idx", "freq", "k", "totals", "b1", "b2")}
        n = self.n if n_files is None else n_files
        t = TEMPLATE1.encode()
        tail = (self.err, self.lib.ERRCAP)
        if symbol == "scg_count_dual_barcodes_diagnostics_files":
            args = (a["paths"], t, 0, 0, self.pool1, a["paths"], t, 0, 0, self.pool2, 2, n, 0, 1, 1,
                    a["counts"], a["idx"], a["freq"], a["k"], a["totals"], a["b1"], a["b2"]) + tail
        elif symbol == "scg_count_combo_barcodes_paired_files":
            args = (a["paths"], t, 0, 0, self.pool1, 2, a["paths"], t, 0, 0, self.pool2, 2, n, 0, 1, 1,
                    a["idx"], a["freq"], a["k"], a["totals"], a["b1"], a["b2"]) + tail
        elif symbol == "scg_count_dual_barcodes_single_end_files":
            args = (a["paths"], n, SE_TEMPLATE.encode(), self.rows, self.sizes, 2, 2, 0, 1, 1, a["counts"], a["totals"]) + tail
        else:
            args = (a["paths"], n, SE_TEMPLATE.encode(), self.rows, self.sizes, 2, 2, 0, 1, 1,
                    a["counts"], a["idx"], a["freq"], a["k"], a["totals"]) + tail
        rc = getattr(self.L, symbol)(*args)
        return rc, self.err.value.decode()


POINTERS = {
    "scg_count_dual_barcodes_diagnostics_files": ("paths", "counts", "idx", "freq", "k", "totals", "b1", "b2"),
    "scg_count_combo_barcodes_paired_files": ("paths", "idx", "freq", "k", "totals", "b1", "b2"),
    "scg_count_dual_barcodes_single_end_files": ("paths", "counts", "totals"),
    "scg_count_dual_barcodes_single_end_diagnostics_files": ("paths", "counts", "idx", "freq", "k", "totals"),
}


@pytest.mark.parametrize("symbol", sorted(POINTERS))
def test_null_arguments(sc, tmp_path, symbol):
    from screencounter_amd import _lib
    raw = Raw(tmp_path)
    for name in POINTERS[symbol]:
        assert raw.call(symbol, without=name) == (_lib.SCG_ERR_INVALID, "null argument"), name
    # a null entry inside the list of paths
    raw.paths[1] = None
    assert raw.call(symbol) == (_lib.SCG_ERR_INVALID, "null argument")
    # a negative number of files
    assert raw.call(symbol, n_files=-1) == (_lib.SCG_ERR_INVALID, "null argument")
    # the caller's pointer arrays are never left with something to free
    assert all(not raw.idx[f] and not raw.freq[f] for f in range(2))
    # no files: nothing is needed, nothing is written
    raw.totals[0] = 77
    for name in (None,) + POINTERS[symbol]:
        assert raw.call(symbol, without=name, n_files=0) == (_lib.SCG_OK, ""), name
    assert raw.totals[0] == 77


def test_failed_calls_leave_the_pointer_arrays_null(sc, tmp_path):
    """Whatever a call fails with (here: no device, or the missing first file), entries f of the caller's arrays are NULL."""
    from screencounter_amd import _lib
    for symbol in sorted(POINTERS):
        if "idx" not in POINTERS[symbol]:
            continue
        raw = Raw(tmp_path)
        junk = (C.c_int32 * 1)()
        for f in range(2):
            raw.idx[f] = C.cast(junk, _lib.i32_p)          # what an uninitialised caller-side array may hold
            raw.freq[f] = C.cast(junk, _lib.i32_p)
            raw.k[f] = 5
        rc, _msg = raw.call(symbol)
        assert rc in (_lib.SCG_ERR_DEVICE, _lib.SCG_ERR_IO), symbol
        assert all(not raw.idx[f] and not raw.freq[f] and raw.k[f] == 0 for f in range(2)), symbol
