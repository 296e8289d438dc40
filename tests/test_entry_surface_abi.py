"""The rest of the many-files contract of include/scg.h without a GPU, next to test_files_entries_abi.py and
test_single_paired_abi.py (which pin the five entries that look at their arguments first): the three entries with a
library that open file 0's reader(s) before they compile, and the random entry, report a missing first file whatever else
is wrong; one file is the one-file entry's business; null arguments, a negative file count and no files for the five
symbols test_files_entries_abi.py does not call raw.  And the Python mirror's unmarshalling of combinations (indices
int32[2, K], freq int32[K], both copies) through combo_compact.

Files are missing unless a test writes them, and every expectation is stated for a machine with and without a device."""
import ctypes as C

import numpy as np
import pytest

SINGLE, COMBO, DUAL, RANDOM = "ACGT----TGCA", "ACGT----TG--CA", "AC--GT", "ACGT----ACGT"
POOL4, POOL2, POOL2B = ["AAAA", "CCCC"], ["CC", "GG"], ["AA", "TT"]


def missing(tmp_path, stem, n=2):
    return [str(tmp_path / f"{stem}{i}.fastq") for i in range(n)]


def error_of(sc, fn, *args):
    with pytest.raises(sc.ScgError) as e:
        fn(*args)
    return e.value.code, str(e.value)


# ---- the reader of file 0 comes before the template and the pools ------------------------------------------------------
def single_files(sc, a, b, template=SINGLE, pool=POOL4):
    return sc.count_single_barcodes_files, (a, template, 2, pool, 0, True, 1)


def combo_single_files(sc, a, b, template=COMBO, pool=(POOL4, POOL2)):
    return sc.count_combo_barcodes_single_files, (a, template, 2, list(pool), 0, True, 1)


def dual_files(sc, a, b, template=DUAL, pool=POOL2):
    return sc.count_dual_barcodes_files, (a, DUAL, False, 0, pool, b, template, False, 0, POOL2B, False, True, 1)


def random_files(sc, a, b, template=RANDOM, pool=None):
    return sc.count_random_barcodes_files, (a, template, 2, 0, True, 1)


PROBE_FIRST = [
    # (entry, what is wrong besides the files: a template or a pool its compile step refuses)
    (single_files, dict(pool=["AAAA", "AAA"])),
    (single_files, dict(template="ACGT--A--TGCA")),
    (combo_single_files, dict(template=SINGLE)),
    (combo_single_files, dict(pool=(["AAAA", "AAAA"], POOL2))),
    (dual_files, dict(template="AC--G-T")),
    (dual_files, dict(pool=["AA", "CCC"])),
    (random_files, dict(template="ACGTACGTAC")),
]


@pytest.mark.parametrize("entry,wrong", PROBE_FIRST, ids=[f"{e.__name__}:{'+'.join(w)}" for e, w in PROBE_FIRST])
def test_missing_first_file_comes_before_the_argument_checks(sc, tmp_path, entry, wrong):
    """As in a loop over the files: SCG_ERR_IO naming file 0, with valid arguments and with arguments compile refuses.
    Once file 0 is there, compile does refuse them -- in the three entries with a library after the device list is read
    (no device: SCG_ERR_DEVICE), in the random entry before it."""
    from screencounter_amd import _lib
    a, b = missing(tmp_path, "a"), missing(tmp_path, "b")
    for kwargs in ({}, wrong):
        fn, args = entry(sc, a, b, **kwargs)
        code, msg = error_of(sc, fn, *args)
        assert code == _lib.SCG_ERR_IO and "a0.fastq" in msg, (kwargs, code, msg)
    for path in (a[0], b[0]):
        with open(path, "wb") as f:
            f.write(b"@r\nACGTAAAATGCA\n+\nIIIIIIIIIIII\n")
    fn, args = entry(sc, a, b, **wrong)
    code, msg = error_of(sc, fn, *args)
    if entry is random_files or sc.load().scg_device_count() > 0:
        assert code == _lib.SCG_ERR_INVALID, (code, msg)
    else:
        assert code == _lib.SCG_ERR_DEVICE and "no HIP device" in msg, (code, msg)


def test_dual_files_opens_both_first_readers(sc, tmp_path):
    from screencounter_amd import _lib
    here = tmp_path / "a0.fastq"
    here.write_bytes(b"@r\nACAAGT\n+\nIIIIII\n")
    fn, args = dual_files(sc, missing(tmp_path, "a"), missing(tmp_path, "b"), template="AC--G-T")
    code, msg = error_of(sc, fn, *args)
    assert code == _lib.SCG_ERR_IO and "b0.fastq" in msg, (code, msg)


@pytest.mark.parametrize("pool", [POOL4, ["AAAA", "AAA"]], ids=["valid pool", "bad pool"])
def test_one_file_is_the_one_file_entry(sc, tmp_path, pool):
    """n_files == 1 delegates: the one-file entry's code and message, here for a file that is not there."""
    from screencounter_amd import _lib
    path = missing(tmp_path, "only", 1)[0]
    one = error_of(sc, sc.count_single_barcodes, path, SINGLE, 2, pool, 0, True, 1)
    assert one[0] == _lib.SCG_ERR_IO and "only0.fastq" in one[1], one
    assert error_of(sc, sc.count_single_barcodes_files, [path], SINGLE, 2, pool, 0, True, 1) == one


# ---- the raw symbols: null arguments, a negative file count, no files ----------------------------------------------------
class Raw:
    """Argument lists of the five symbols with every pointer in place; `without` nulls one of them by name."""
    POINTERS = {
        "scg_count_single_barcodes_files": ("paths1", "counts", "totals"),
        "scg_count_combo_barcodes_single_files": ("paths1", "idx", "freq", "k", "totals"),
        "scg_count_dual_barcodes_files": ("paths1", "paths2", "counts", "totals"),
        "scg_count_single_barcodes_paired_files": ("paths1", "paths2", "counts", "totals"),
        "scg_count_random_barcodes_files": ("paths1", "totals"),
    }
    RANDOM_OUTPUTS = ("seq", "nkeys", "vlen", "col", "rows", "rfreq")       # needed whatever n_files is

    def __init__(self, tmp_path):
        from screencounter_amd import _lib
        self.lib, self.L = _lib, _lib.load()
        self.paths1, self._k1 = _lib.cstr_array(missing(tmp_path, "a"))
        self.paths2, self._k2 = _lib.cstr_array(missing(tmp_path, "b"))
        self.pool4, self._k3 = _lib.cstr_array(POOL4)
        self.pool2, self._k4 = _lib.cstr_array(POOL2)
        self.pool2b, self._k5 = _lib.cstr_array(POOL2B)
        self.counts, self.totals = (C.c_int32 * 8)(), (C.c_int32 * 2)()
        self.idx, self.freq, self.k = (_lib.i32_p * 2)(), (_lib.i32_p * 2)(), (C.c_int64 * 2)()
        self.seq, self.nkeys, self.vlen = C.pointer(C.c_void_p()), C.pointer(C.c_int64(-1)), C.pointer(C.c_int32(-1))
        self.col, self.rows, self.rfreq = C.pointer(_lib.i64_p()), C.pointer(_lib.i32_p()), C.pointer(_lib.i32_p())
        self.err = _lib.errbuf()

    def call(self, symbol, without=None, n_files=2):
        a = {name: (None if name == without else getattr(self, name))
             for name in ("paths1", "paths2", "counts", "totals", "idx", "freq", "k") + self.RANDOM_OUTPUTS}
        tail = (self.err, self.lib.ERRCAP)
        if symbol == "scg_count_single_barcodes_files":
            args = (a["paths1"], n_files, SINGLE.encode(), 2, self.pool4, 2, 0, 1, 1, a["counts"], a["totals"])
        elif symbol == "scg_count_combo_barcodes_single_files":
            args = (a["paths1"], n_files, COMBO.encode(), 2, self.pool4, 2, self.pool2, 2, 0, 1, 1, a["idx"], a["freq"], a["k"], a["totals"])
        elif symbol == "scg_count_dual_barcodes_files":
            args = (a["paths1"], DUAL.encode(), 0, 0, self.pool2, a["paths2"], DUAL.encode(), 0, 0, self.pool2b, 2, n_files, 0, 1, 1,
                    a["counts"], a["totals"])
        elif symbol == "scg_count_single_barcodes_paired_files":
            args = (a["paths1"], a["paths2"], n_files, SINGLE.encode(), 2, self.pool4, 2, 0, 1, 1, a["counts"], a["totals"])
        else:
            args = (a["paths1"], n_files, RANDOM.encode(), 2, 0, 1, 1, a["seq"], a["nkeys"], a["vlen"], a["col"], a["rows"], a["rfreq"],
                    a["totals"])
        rc = getattr(self.L, symbol)(*(args + tail))
        return rc, self.err.value.decode()

    def release_random(self):
        for p in (self.seq, self.col, self.rows, self.rfreq):
            self.L.scg_free(p.contents)


@pytest.mark.parametrize("symbol", sorted(Raw.POINTERS))
def test_null_arguments(sc, tmp_path, symbol):
    from screencounter_amd import _lib
    null = (_lib.SCG_ERR_INVALID, "null argument")
    is_random = symbol == "scg_count_random_barcodes_files"
    raw = Raw(tmp_path)
    for name in Raw.POINTERS[symbol] + (Raw.RANDOM_OUTPUTS if is_random else ()):
        assert raw.call(symbol, without=name) == null, name
    # a negative number of files
    assert raw.call(symbol, n_files=-1) == null
    # a null entry inside a list of paths, second and first
    for f in (1, 0):
        raw.paths1[f] = None
        assert raw.call(symbol) == null, f
    # no files: the arrays of n_files entries are not needed, and nothing is written to them
    raw.totals[0] = 77
    for name in (None,) + Raw.POINTERS[symbol]:
        assert raw.call(symbol, without=name, n_files=0) == (_lib.SCG_OK, ""), name
        if is_random:                          # (an empty matrix, with its four arrays to release)
            assert raw.nkeys.contents.value == 0 and raw.seq.contents.value and raw.col.contents[0] == 0
            raw.release_random()
    assert raw.totals[0] == 77
    if is_random:                              # its own outputs are needed whatever the number of files
        for name in Raw.RANDOM_OUTPUTS:
            assert raw.call(symbol, without=name, n_files=0) == null, name


def test_a_failed_combo_call_leaves_the_pointer_arrays_null(sc, tmp_path):
    """Whatever the call fails with (the missing first file; a null path), entries f of the caller's arrays are NULL, k 0."""
    from screencounter_amd import _lib
    for null_path in (False, True):
        raw = Raw(tmp_path)
        junk = (C.c_int32 * 1)()
        for f in range(2):
            raw.idx[f] = C.cast(junk, _lib.i32_p)              # what an uninitialised caller-side array may hold
            raw.freq[f] = C.cast(junk, _lib.i32_p)
            raw.k[f] = 5
        if null_path:
            raw.paths1[1] = None
        rc, _msg = raw.call("scg_count_combo_barcodes_single_files")
        assert rc == (_lib.SCG_ERR_INVALID if null_path else _lib.SCG_ERR_IO)
        assert all(not raw.idx[f] and not raw.freq[f] and raw.k[f] == 0 for f in range(2))


# ---- combinations as the mirror hands them out -------------------------------------------------------------------------------
COMPACT = [
    ("no cell", [[0, 0], [0, 0], [0, 0]], np.zeros((2, 0), dtype=np.int32), []),
    ("one cell", [[0, 0], [0, 0], [0, 5]], [[2], [1]], [5]),
    ("3 x 2", [[1, 0], [0, 2], [3, 4]], [[0, 1, 2, 2], [0, 1, 0, 1]], [1, 2, 3, 4]),
]


@pytest.mark.parametrize("cells,indices,freq", [c[1:] for c in COMPACT], ids=[c[0] for c in COMPACT])
def test_combinations_are_unmarshalled_as_owned_int32_arrays(sc, cells, indices, freq):
    got_indices, got_freq = sc.combo_compact(np.array(cells, dtype=np.int32), 3, 2)
    K = len(freq)
    assert got_indices.shape == (2, K) and got_freq.shape == (K,)
    assert got_indices.dtype == np.int32 and got_freq.dtype == np.int32
    assert got_indices.tolist() == np.asarray(indices).reshape(2, K).tolist() and got_freq.tolist() == freq
    for arr in (got_indices, got_freq):                      # copies that own their memory: the C side's arrays are gone
        assert arr.flags.owndata and arr.base is None
