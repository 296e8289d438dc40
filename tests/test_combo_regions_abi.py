"""Combinations over any number of variable regions (kaori::CombinatorialBarcodesSingleEnd<N, V>, V = 1..8) without a GPU:
the new symbols exist, and their host-side half -- compile_combo_regions -- raises every argument error with its exact
text, in the stated order, before any device work: null arguments, the number of regions this engine takes, the pools'
own errors, the handler's constructor checks in its order, the budget, the product of the pool sizes.  The one-file entry
opens its reader first; the two-region entry keeps its own message."""
import ctypes as C
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ("scg_plan_combo_regions", "scg_count_combo_barcodes_regions", "scg_count_combo_barcodes_regions_files")
T3 = "ACGT----TG---CA-----GT"            # regions of 4, 3 and 5 bases
P3 = [["AAAA", "CCCC"], ["AAA", "CCC", "GGG"], ["AAAAA"]]
RANGE = "this engine counts combinations of 1 to 8 variable regions (got %d)"


def error_of(sc, fn, *args, **kwargs):
    with pytest.raises(sc.ScgError) as e:
        fn(*args, **kwargs)
    return e.value.code, str(e.value)


def has_device(sc):
    return sc.load().scg_device_count() > 0


@pytest.fixture
def one_read(tmp_path):
    p = tmp_path / "one.fastq"
    p.write_bytes(b"@r\nACGTAAAATGCCCCAAAAAAGT\n+\nIIIIIIIIIIIIIIIIIIIIII\n")
    return str(p)


def every_entry(sc, tmp_path, one_read, template, strand, pools, mismatches=0):
    """The error of the plan, of the one-file entry on a file that exists, and of the many-files entry on two that do: one
    (code, message) for all three."""
    got = error_of(sc, sc.Plan.combo_regions, template, strand, pools, mismatches)
    assert got == error_of(sc, sc.count_combo_barcodes_regions, one_read, template, strand, pools, mismatches, True)
    assert got == error_of(sc, sc.count_combo_barcodes_regions_files, [one_read, one_read], template, strand, pools, mismatches, True)
    return got


def test_symbols_are_declared_exported_and_bound(sc):
    from screencounter_amd import _lib
    header = open(os.path.join(ROOT, "include", "scg.h")).read()
    lib = sc.load()
    for name in SYMBOLS:
        assert re.search(r"\bint " + name + r"\(", header), name
        assert hasattr(lib, name) and name in _lib.SIGNATURES, name
    assert re.search(r"\bint32_t scg_plan_num_regions\(", header) and hasattr(lib, "scg_plan_num_regions") and "scg_plan_num_regions" in _lib.SIGNATURES
    assert all(hasattr(sc, name) for name in ("count_combo_barcodes_regions", "count_combo_barcodes_regions_files"))
    assert hasattr(sc.Plan, "combo_regions") and hasattr(sc.Plan, "read_combinations")
    assert lib.scg_plan_num_regions(None) == 0


BAD = [
    # (code name, exact message, template, pools, mismatches)
    ("SCG_ERR_INVALID", "expected 3 variable regions in the constant template", "ACGT----TG---CA", P3, 0),
    ("SCG_ERR_INVALID", "expected 2 variable regions in the constant template", T3, P3[:2], 0),
    ("SCG_ERR_INVALID", "expected 1 variable regions in the constant template", "ACGTACGT", [["AAAA"]], 0),
    ("SCG_ERR_INVALID", "length of variable region 1 (4) should be the same as its sequences (5)", T3, [["AAAAA"], P3[1], P3[2]], 0),
    ("SCG_ERR_INVALID", "length of variable region 2 (3) should be the same as its sequences (4)", T3, [P3[0], ["AAAA"], P3[2]], 0),
    ("SCG_ERR_INVALID", "length of variable region 3 (5) should be the same as its sequences (0)", T3, [P3[0], P3[1], []], 0),
    ("SCG_ERR_INVALID", "negative number of mismatches", T3, P3, -1),
]


@pytest.mark.parametrize("code,message,template,pools,mismatches", BAD, ids=[f"{i}" for i in range(len(BAD))])
def test_constructor_errors_carry_their_exact_text(sc, tmp_path, one_read, code, message, template, pools, mismatches):
    from screencounter_amd import _lib
    assert every_entry(sc, tmp_path, one_read, template, 2, pools, mismatches) == (getattr(_lib, code), message)


def test_errors_come_in_the_stated_order(sc, tmp_path, one_read):
    """Everything wrong at once, then one fault fewer each time: the number of regions this engine takes; the pools' own
    errors (unequal lengths); the template's; the number of regions in the template; the regions' lengths, first region
    first; the budget; the product of the pool sizes."""
    from screencounter_amd import _lib
    INV, UNS = _lib.SCG_ERR_INVALID, _lib.SCG_ERR_UNSUPPORTED
    nine = [["AAAA", "AAA"]] * 9
    assert every_entry(sc, tmp_path, one_read, "ACXT----", 2, nine, -1) == (UNS, RANGE % 9)
    ragged = [["AAAA", "AAA"], ["AAAA"], ["AAAA"]]
    code, msg = every_entry(sc, tmp_path, one_read, "ACXT----", 2, ragged, -1)
    assert code == INV and "same length" in msg
    even = [["AAAAA"], ["AAAA"], ["AAAAAA"]]
    code, msg = every_entry(sc, tmp_path, one_read, "ACXT----", 0, even, -1)
    assert code == INV and "unknown base 'X'" in msg
    assert every_entry(sc, tmp_path, one_read, "ACGT----", 2, even, -1) == (INV, "expected 3 variable regions in the constant template")
    assert every_entry(sc, tmp_path, one_read, T3, 2, even, -1) == (INV, "length of variable region 1 (4) should be the same as its sequences (5)")
    assert every_entry(sc, tmp_path, one_read, T3, 2, [["AAAA"], ["AAAA"], ["AAAAAA"]], -1) == (INV, "length of variable region 2 (3) should be the same as its sequences (4)")
    assert every_entry(sc, tmp_path, one_read, T3, 2, [["AAAA"], ["AAA"], ["AAAAAA"]], -1) == (INV, "length of variable region 3 (5) should be the same as its sequences (6)")
    assert every_entry(sc, tmp_path, one_read, T3, 2, [["AAAA"], ["AAA"], ["AAAAA"]], -1) == (INV, "negative number of mismatches")
    # a library's own error (duplicates) comes when the libraries are built: after the constructor's checks
    code, msg = every_entry(sc, tmp_path, one_read, T3, 2, [["AAAA", "AAAA"], ["AAA"], ["AAAAA"]], 0)
    assert code == INV and re.search(r"duplicate sequences detected \(1, 2\)", msg)


def test_region_counts_outside_1_to_8(sc, tmp_path, one_read):
    from screencounter_amd import _lib
    assert every_entry(sc, tmp_path, one_read, "ACGTACGT", 2, []) == (_lib.SCG_ERR_UNSUPPORTED, RANGE % 0)
    t9 = "A".join(["---"] * 9)
    assert every_entry(sc, tmp_path, one_read, t9, 2, [["AAA"]] * 9) == (_lib.SCG_ERR_UNSUPPORTED, RANGE % 9)


def test_product_of_the_pool_sizes_must_stay_below_2_to_63(sc, tmp_path, one_read):
    """Eight pools of 300 sequences: 300^8 = 6.6e19 > 2^63 = 9.2e18 (300^7 = 2.2e17 still fits).  Checked with overflow
    checks before any index is built, so the message is not the wrapped product's."""
    from screencounter_amd import _lib
    import itertools
    pool = ["".join(p) for p in itertools.islice(itertools.product("ACGT", repeat=5), 300)]
    t8 = "A".join(["-----"] * 8)
    code, msg = every_entry(sc, tmp_path, one_read, t8, 0, [pool] * 8)
    assert code == _lib.SCG_ERR_UNSUPPORTED and "2^63 combinations or more" in msg, (code, msg)
    # 2^8 sequences in each of eight pools: 2^64 combinations, which is 0 in 64 bits
    pool256 = ["".join(p) for p in itertools.product("ACGT", repeat=4)]
    code, msg = every_entry(sc, tmp_path, one_read, "A".join(["----"] * 8), 0, [pool256] * 8)
    assert code == _lib.SCG_ERR_UNSUPPORTED and "2^63 combinations or more" in msg, (code, msg)
    t7 = "A".join(["-----"] * 7)
    if has_device(sc):
        with sc.Plan.combo_regions(t7, 0, [pool] * 7) as p:
            assert p.num_counters == 0                            # (a key stream, no cells)
    else:
        code, msg = error_of(sc, sc.Plan.combo_regions, t7, 0, [pool] * 7)
        assert code == _lib.SCG_ERR_DEVICE and "no HIP device" in msg, (code, msg)


def test_a_missing_file_is_reported_before_the_arguments(sc, tmp_path, one_read):
    from screencounter_amd import _lib
    nope = str(tmp_path / "nope.fastq")
    code, msg = error_of(sc, sc.count_combo_barcodes_regions, nope, "ACGT----", 2, P3, -1, True)
    assert code == _lib.SCG_ERR_IO and "failed to open file" in msg, (code, msg)
    code, msg = error_of(sc, sc.count_combo_barcodes_regions_files, [nope, one_read], "ACGT----", 2, P3, -1, True)
    assert code == _lib.SCG_ERR_IO and "failed to open file" in msg, (code, msg)
    # ... of the FIRST file only: a later one is met after the arguments
    code, msg = error_of(sc, sc.count_combo_barcodes_regions_files, [one_read, nope], "ACGT----", 2, P3, 0, True)
    assert (code, msg) == (_lib.SCG_ERR_INVALID, "expected 3 variable regions in the constant template")


def test_null_arguments_are_rejected(sc, one_read):
    from screencounter_amd import _lib
    L = sc.load()
    err = C.create_string_buffer(256)
    rows, sizes, _keep = _lib.cstr_matrix(P3)
    idx, freq, k, total, plan = _lib.i32_p(), _lib.i32_p(), C.c_int64(0), C.c_int32(0), C.c_void_p()
    outs = (C.byref(idx), C.byref(freq), C.byref(k), C.byref(total))
    path, tmpl = one_read.encode(), T3.encode()

    def null(rc):
        assert (rc, err.value) == (_lib.SCG_ERR_INVALID, b"null argument"), (rc, err.value)
    null(L.scg_plan_combo_regions(C.byref(plan), None, 2, rows, sizes, 3, 0, 1, -1, err, 256))
    null(L.scg_plan_combo_regions(C.byref(plan), tmpl, 2, None, sizes, 3, 0, 1, -1, err, 256))
    null(L.scg_plan_combo_regions(C.byref(plan), tmpl, 2, rows, None, 3, 0, 1, -1, err, 256))
    holes = (_lib.c_str_p * 3)(rows[0], None, rows[2])
    null(L.scg_plan_combo_regions(C.byref(plan), tmpl, 2, holes, sizes, 3, 0, 1, -1, err, 256))
    negative = (C.c_int32 * 3)(2, -1, 1)
    null(L.scg_plan_combo_regions(C.byref(plan), tmpl, 2, rows, negative, 3, 0, 1, -1, err, 256))
    null(L.scg_count_combo_barcodes_regions(None, tmpl, 2, rows, sizes, 3, 0, 1, 1, *outs, err, 256))
    null(L.scg_count_combo_barcodes_regions(path, None, 2, rows, sizes, 3, 0, 1, 1, *outs, err, 256))
    null(L.scg_count_combo_barcodes_regions(path, tmpl, 2, None, sizes, 3, 0, 1, 1, *outs, err, 256))
    for hole in range(4):
        args = list(outs)
        args[hole] = None
        null(L.scg_count_combo_barcodes_regions(path, tmpl, 2, rows, sizes, 3, 0, 1, 1, *args, err, 256))
    files = (C.c_char_p * 2)(path, path)
    idxs, freqs, ks, totals = (_lib.i32_p * 2)(), (_lib.i32_p * 2)(), (C.c_int64 * 2)(), (C.c_int32 * 2)()
    null(L.scg_count_combo_barcodes_regions_files(None, 2, tmpl, 2, rows, sizes, 3, 0, 1, 1, idxs, freqs, ks, totals, err, 256))
    null(L.scg_count_combo_barcodes_regions_files(files, -1, tmpl, 2, rows, sizes, 3, 0, 1, 1, idxs, freqs, ks, totals, err, 256))
    null(L.scg_count_combo_barcodes_regions_files(files, 2, tmpl, 2, rows, sizes, 3, 0, 1, 1, None, freqs, ks, totals, err, 256))
    null(L.scg_count_combo_barcodes_regions_files(files, 2, tmpl, 2, rows, sizes, 3, 0, 1, 1, idxs, freqs, ks, None, err, 256))
    null(L.scg_count_combo_barcodes_regions_files((C.c_char_p * 2)(path, None), 2, tmpl, 2, rows, sizes, 3, 0, 1, 1, idxs, freqs, ks, totals, err, 256))
    assert L.scg_count_combo_barcodes_regions_files(files, 0, tmpl, 2, rows, sizes, 3, 0, 1, 1, idxs, freqs, ks, totals, err, 256) == _lib.SCG_OK
    rc = L.scg_plan_read_combinations(None, C.byref(idx), C.byref(freq), C.byref(k), None, None, err, 256)
    null(rc)


def test_valid_arguments_need_a_device_or_work(sc, one_read):
    from screencounter_amd import _lib
    if has_device(sc):
        with sc.Plan.combo_regions(T3, 2, P3, 1, False) as p:
            assert p.kind == "combo_regions" and p.n_pool == (2, 3, 1) and p.num_counters == 6
            assert sc.load().scg_plan_num_regions(p._h) == 3
    else:
        for fn, args in ((sc.Plan.combo_regions, (T3, 2, P3, 1, False)), (sc.count_combo_barcodes_regions, (one_read, T3, 2, P3, 1, False)),
                         (sc.count_combo_barcodes_regions_files, ([one_read, one_read], T3, 2, P3, 1, False))):
            code, msg = error_of(sc, fn, *args)
            assert code == _lib.SCG_ERR_DEVICE and "no HIP device" in msg, (code, msg)


def test_the_two_region_entry_still_refuses_three_pools(sc, one_read):
    """The entries of countComboBarcodes keep the reference's own limit and text (src/count_combo_barcodes_single.cpp:44-46)."""
    from screencounter_amd import _lib
    want = (_lib.SCG_ERR_INVALID, "currently expecting only 2 variable regions for single-end combinatorial barcodes")
    assert error_of(sc, sc.count_combo_barcodes_single, one_read, T3, 2, P3, 0, True) == want
    assert error_of(sc, sc.count_combo_barcodes_single_files, [one_read, one_read], T3, 2, P3, 0, True) == want
    code, msg = error_of(sc, sc.Plan.combo, T3, 2, P3[0], P3[1], 0, True)
    assert (code, msg) == (_lib.SCG_ERR_INVALID, "expected 2 variable regions in the constant template")
