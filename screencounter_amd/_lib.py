"""ctypes binding of libscg.so (include/scg.h).

The shared library is built in-tree by ``__graft_entry__.build()`` (or ``make -C
screencounter_amd/csrc``).  There is no fallback of any kind: if the library is missing the
import fails, and if no HIP device is present every counting call returns SCG_ERR_DEVICE.

Besides the signatures: the marshalling steps that api.py and engine.py share, each written once -- strings and pools in
(cstr_array, pool, cstr_matrix), combinations out (combo_outputs, per_file_combo_outputs, combo_matrix_outputs) and sequence blobs out
(decode_sequences).
"""
from __future__ import annotations

import contextlib
import ctypes as C
import os

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("SCG_LIB") or os.path.join(_HERE, "libscg.so")     # SCG_LIB: A/B builds (tools/ab.sh)

SCG_OK, SCG_ERR_INVALID, SCG_ERR_IO, SCG_ERR_DEVICE, SCG_ERR_UNSUPPORTED = 0, 1, 2, 3, 4
ERRCAP = 1024

c_str_p = C.POINTER(C.c_char_p)
i32_p = C.POINTER(C.c_int32)
i64_p = C.POINTER(C.c_int64)


class SynthSpec(C.Structure):
    """struct scg_synth_spec (include/scg.h)"""
    _fields_ = [
        ("seed", C.c_uint64),
        ("first_read", C.c_int64),
        ("read_len", C.c_int32),
        ("template_len", C.c_int32),
        ("d_template", C.c_void_p),
        ("n_regions", C.c_int32),
        ("region_start", C.c_int32 * 2),
        ("region_len", C.c_int32 * 2),
        ("d_pool", C.c_void_p * 2),
        ("n_pool", C.c_int32 * 2),
        ("d_pair_index", C.c_void_p),
        ("n_pairs", C.c_int32),
        ("pair_column", C.c_int32),
        ("p_invalid_pair", C.c_float),
        ("p_sub", C.c_float),
        ("p_n", C.c_float),
        ("p_junk", C.c_float),
        ("p_reverse", C.c_float),
    ]


# Argument groups that recur in include/scg.h, so that a row below reads like the header's prototype.
STR, INT, I32, I64, PTR = C.c_char_p, C.c_int, C.c_int32, C.c_int64, C.c_void_p
ERR = [STR, C.c_size_t]                           # char* err, size_t errcap
POOL = [c_str_p, I32]                             # const char* const* pool, int32_t n_pool
POOLS = [C.POINTER(c_str_p), i32_p, I32]          # const char* const* const* pools, const int32_t* n_pools, int32_t n_regions
COMBOS = [C.POINTER(i32_p), C.POINTER(i32_p), i64_p]     # int32_t** indices_out, int32_t** freq_out, int64_t* k_out (one entry, or one per file)
# int32_t** indices_out, int64_t* k_out, int64_t** col_ptr_out, int32_t** rows_out, int32_t** freq_out (the combination matrix)
MATRIX = [C.POINTER(i32_p), i64_p, C.POINTER(i64_p), C.POINTER(i32_p), C.POINTER(i32_p)]
READS = [PTR, PTR, I32]                          # const char* d_seqs, const uint32_t* d_offsets, int32_t fixed_len
PLAN_OUT = C.POINTER(PTR)                         # scg_plan** plan_out

# name -> (restype, argtypes); must list every symbol declared in include/scg.h
SIGNATURES = {
    "scg_version": (STR, []),
    "scg_device_count": (INT, []),
    "scg_set_device": (INT, [INT, *ERR]),
    "scg_set_devices": (INT, [C.POINTER(INT), INT, *ERR]),
    "scg_count_single_barcodes": (INT, [STR, STR, INT, *POOL, INT, INT, INT, i32_p, i32_p, *ERR]),
    "scg_count_combo_barcodes_single": (INT, [STR, STR, INT, *POOL, *POOL, INT, INT, INT, *COMBOS, i32_p, *ERR]),
    "scg_count_dual_barcodes": (INT, [STR, STR, INT, INT, c_str_p, STR, STR, INT, INT, c_str_p, I32,
                                      INT, INT, INT, INT, i32_p, i32_p, *ERR]),
    "scg_count_combo_barcodes_regions": (INT, [STR, STR, INT, *POOLS, INT, INT, INT, *COMBOS, i32_p, *ERR]),
    "scg_count_combo_barcodes_regions_files": (INT, [c_str_p, I32, STR, INT, *POOLS, INT, INT, INT, *COMBOS, i32_p, *ERR]),
    "scg_count_single_barcodes_paired": (INT, [STR, STR, STR, INT, *POOL, INT, INT, INT, i32_p, i32_p, *ERR]),
    "scg_count_single_barcodes_paired_files": (INT, [c_str_p, c_str_p, I32, STR, INT, *POOL, INT, INT, INT, i32_p, i32_p, *ERR]),
    "scg_match_barcodes": (INT, [*POOL, *POOL, INT, INT, i32_p, i32_p, *ERR]),
    "scg_count_single_barcodes_files": (INT, [c_str_p, I32, STR, INT, *POOL, INT, INT, INT, i32_p, i32_p, *ERR]),
    "scg_count_combo_barcodes_single_files": (INT, [c_str_p, I32, STR, INT, *POOL, *POOL, INT, INT, INT, *COMBOS, i32_p, *ERR]),
    "scg_count_dual_barcodes_files": (INT, [c_str_p, STR, INT, INT, c_str_p, c_str_p, STR, INT, INT, c_str_p, I32, I32,
                                            INT, INT, INT, i32_p, i32_p, *ERR]),
    "scg_count_dual_barcodes_diagnostics_files": (INT, [c_str_p, STR, INT, INT, c_str_p, c_str_p, STR, INT, INT, c_str_p, I32, I32,
                                                        INT, INT, INT, i32_p, *COMBOS, i32_p, i32_p, i32_p, *ERR]),
    "scg_count_dual_barcodes_single_end_files": (INT, [c_str_p, I32, STR, *POOLS, INT, INT, INT, INT, i32_p, i32_p, *ERR]),
    "scg_count_dual_barcodes_single_end_diagnostics_files": (INT, [c_str_p, I32, STR, *POOLS, INT, INT, INT, INT, i32_p, *COMBOS, i32_p, *ERR]),
    "scg_count_combo_barcodes_paired_files": (INT, [c_str_p, STR, INT, INT, *POOL, c_str_p, STR, INT, INT, *POOL, I32,
                                                    INT, INT, INT, *COMBOS, i32_p, i32_p, i32_p, *ERR]),
    "scg_count_random_barcodes_files": (INT, [c_str_p, I32, STR, INT, INT, INT, INT,
                                              C.POINTER(PTR), i64_p, i32_p, C.POINTER(i64_p), C.POINTER(i32_p), C.POINTER(i32_p), i32_p, *ERR]),
    "scg_combine_combinations": (INT, [C.POINTER(i32_p), C.POINTER(i32_p), i64_p, I32, *MATRIX, *ERR]),
    "scg_count_combo_barcodes_single_matrix": (INT, [c_str_p, I32, STR, INT, *POOL, *POOL, INT, INT, INT, *MATRIX, i32_p, *ERR]),
    "scg_count_combo_barcodes_paired_matrix": (INT, [c_str_p, STR, INT, INT, *POOL, c_str_p, STR, INT, INT, *POOL, I32,
                                                     INT, INT, INT, *MATRIX, i32_p, i32_p, i32_p, *ERR]),
    "scg_combo_compact_device": (INT, [i32_p, I32, I32, *COMBOS, *ERR]),
    "scg_fastq_text_windows": (INT, [STR, I64, INT, C.POINTER(PTR), i64_p, C.POINTER(PTR), i64_p, STR, *ERR]),
    "scg_fastq_scan_windows": (INT, [STR, I64, INT, C.POINTER(PTR), C.POINTER(PTR), i64_p, i64_p, *ERR]),
    "scg_bgzf_member_batches": (INT, [STR, I64, I64, INT, C.POINTER(PTR), i64_p, C.POINTER(PTR), i64_p, i64_p, *ERR]),
    "scg_free": (None, [PTR]),
    "scg_release_buffers": (None, []),
    "scg_parse_fastq": (INT, [STR, C.POINTER(PTR), C.POINTER(PTR), i64_p, *ERR]),
    "scg_plan_single": (INT, [PLAN_OUT, STR, INT, *POOL, INT, INT, INT, *ERR]),
    "scg_plan_single_paired": (INT, [PLAN_OUT, STR, INT, *POOL, INT, INT, INT, *ERR]),
    "scg_plan_combo": (INT, [PLAN_OUT, STR, INT, *POOL, *POOL, INT, INT, INT, *ERR]),
    "scg_plan_combo_regions": (INT, [PLAN_OUT, STR, INT, *POOLS, INT, INT, INT, *ERR]),
    "scg_plan_num_regions": (I32, [PTR]),
    "scg_plan_dual": (INT, [PLAN_OUT, STR, INT, INT, c_str_p, STR, INT, INT, c_str_p, I32, INT, INT, INT, INT, *ERR]),
    "scg_count_dual_barcodes_diagnostics": (INT, [STR, STR, INT, INT, c_str_p, STR, STR, INT, INT, c_str_p, I32,
                                                  INT, INT, INT, i32_p, *COMBOS, i32_p, i32_p, i32_p, *ERR]),
    "scg_count_random_barcodes": (INT, [STR, STR, INT, INT, INT, INT, C.POINTER(PTR), C.POINTER(i32_p), i64_p, i32_p, i32_p, *ERR]),
    "scg_count_dual_barcodes_single_end": (INT, [STR, STR, *POOLS, INT, INT, INT, INT, INT, i32_p, i32_p, *ERR]),
    "scg_count_dual_barcodes_single_end_diagnostics": (INT, [STR, STR, *POOLS, INT, INT, INT, INT, i32_p, *COMBOS, i32_p, *ERR]),
    "scg_plan_dual_single_end": (INT, [PLAN_OUT, STR, INT, *POOLS, INT, INT, INT, *ERR]),
    "scg_count_combo_barcodes_paired": (INT, [STR, STR, INT, INT, *POOL, STR, STR, INT, INT, *POOL,
                                              INT, INT, INT, *COMBOS, i32_p, i32_p, i32_p, *ERR]),
    "scg_plan_paired_combo": (INT, [PLAN_OUT, STR, INT, INT, *POOL, STR, INT, INT, *POOL, INT, INT, INT, *ERR]),
    "scg_plan_read_diagnostics": (INT, [PTR, i32_p, *COMBOS, i64_p, i32_p, i32_p, PTR, *ERR]),
    "scg_plan_random": (INT, [PLAN_OUT, STR, INT, INT, INT, INT, *ERR]),
    "scg_plan_read_random": (INT, [PTR, C.POINTER(PTR), C.POINTER(i32_p), i64_p, i32_p, i64_p, PTR, *ERR]),
    "scg_plan_destroy": (None, [PTR]),
    "scg_plan_num_counters": (I64, [PTR]),
    "scg_plan_device_counters": (PTR, [PTR]),
    "scg_plan_bind_counters": (INT, [PTR, PTR, *ERR]),
    "scg_plan_reset": (INT, [PTR, PTR, *ERR]),
    "scg_count_batch": (INT, [PTR, *READS, I32, I64, PTR, *ERR]),
    "scg_count_batch_paired": (INT, [PTR, *READS, *READS, I32, I64, PTR, *ERR]),
    "scg_assign_batch": (INT, [PTR, *READS, I32, I64, PTR, PTR, PTR, PTR, PTR, PTR, *ERR]),
    "scg_plan_read": (INT, [PTR, i32_p, i64_p, PTR, *ERR]),
    "scg_plan_read_combinations": (INT, [PTR, *COMBOS, i64_p, PTR, *ERR]),
    "scg_combo_compact": (INT, [i32_p, I32, I32, *COMBOS, *ERR]),
    "scg_plan_set_profiling": (INT, [PTR, INT]),
    "scg_plan_kernel_stats": (INT, [PTR, C.POINTER(C.c_double), i64_p, *ERR]),
    "scg_synth_reads": (INT, [C.POINTER(SynthSpec), PTR, I64, PTR, *ERR]),
}

_lib = None


def load() -> C.CDLL:
    """Load libscg.so once.  torch is imported first so that both share one HIP runtime
    (torch ships its own libamdhip64.so.7; whichever is loaded first serves both)."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise ImportError(
            f"{LIB_PATH} is missing: build it with `python -c 'import __graft_entry__ as g; g.build()'` "
            "or `make -C screencounter_amd/csrc`.  screencounter_amd has no CPU fallback.")
    try:
        import torch  # noqa: F401  (loads the HIP runtime torch tensors live in)
    except Exception:  # pragma: no cover - torch is plumbing only; the library works without it
        pass
    lib = C.CDLL(LIB_PATH)
    for name, (res, args) in SIGNATURES.items():
        if os.environ.get("SCG_LIB") and not hasattr(lib, name):
            continue              # an older build under tools/ab/ (A/B timing of entry points both builds have)
        fn = getattr(lib, name)   # AttributeError here means the .so is stale: rebuild
        fn.restype = res
        fn.argtypes = args
    _lib = lib
    return lib


class ScgError(RuntimeError):
    """Non-zero return from libscg; `.code` is one of the SCG_ERR_* values.  SCG_ERR_INVALID /
    SCG_ERR_IO correspond to the std::runtime_error the reference throws (an R error)."""

    def __init__(self, code: int, message: str):
        super().__init__(message)
        self.code = code


def check(rc: int, err) -> None:
    if rc != SCG_OK:
        raise ScgError(rc, err.value.decode(errors="replace"))


def errbuf():
    return C.create_string_buffer(ERRCAP)


def cstr_matrix(pools):
    """list of pools -> (const char* const* const*, int32[] sizes, keepalive) for scg_*_dual_single_end"""
    keep = []
    rows = (c_str_p * max(len(pools), 1))()
    for r, p in enumerate(pools):
        arr, k = cstr_array(p)
        keep.append((arr, k))
        rows[r] = C.cast(arr, c_str_p)
    sizes = (C.c_int32 * max(len(pools), 1))(*[len(p) for p in pools])
    return rows, sizes, keep


class PreparedPool(list):
    """A barcode pool whose C string array has been built once (`prepare_pool`): passing it to the count_* functions
    skips the per-call marshalling of this Python mirror (~0.4 us per barcode; R hands the C side its CHARSXP pointers
    without such a copy)."""
    _carr = None
    _keep = None


def prepare_pool(strings) -> PreparedPool:
    p = PreparedPool(strings)
    p._carr, p._keep = cstr_array(list(strings))
    return p


def cstr_array(strings):
    if isinstance(strings, PreparedPool) and strings._carr is not None:
        return strings._carr, strings._keep
    arr = (C.c_char_p * max(len(strings), 1))()
    keep = []
    for i, s in enumerate(strings):
        b = s.encode() if isinstance(s, str) else bytes(s)
        keep.append(b)
        arr[i] = b
    return arr, keep


def pool(strings):
    """A pool as the header takes it: (const char* const* pool, int32_t n_pool).  (The array holds on to its strings.)"""
    return cstr_array(strings)[0], len(strings)


@contextlib.contextmanager
def per_file_combo_outputs(L, n: int, rows: int = 2):
    """The caller-allocated arrays of n entries for the malloc'd combinations of a many-files entry (int32_t** indices_out,
    int32_t** freq_out, int64_t* k_out).  `with ... as (outputs, take)`: pass `*outputs` to the call; after it, take() is a
    list of n (indices int32[2, K_f], freq int32[K_f]), fresh arrays that own their memory, (2, 0) and (0,) where K_f is 0.
    rows: the rows of the index matrices where they are not 2 (combinations over `rows` variable regions).
    Leaving the block frees every pointer the C side handed out, whatever happened inside: a call that failed, an
    exception while copying."""
    idx, freq, ks = (i32_p * max(n, 1))(), (i32_p * max(n, 1))(), (C.c_int64 * max(n, 1))()

    def copies(f):
        K = int(ks[f])
        if K == 0:                                   # (nothing to read: the pointers are not looked at)
            return np.zeros((rows, 0), dtype=np.int32), np.zeros(0, dtype=np.int32)
        return np.ctypeslib.as_array(idx[f], shape=(K, rows)).T.copy(), np.ctypeslib.as_array(freq[f], shape=(K,)).copy()
    try:
        yield (idx, freq, ks), lambda: [copies(f) for f in range(n)]
    finally:
        for f in range(n):
            L.scg_free(idx[f])
            L.scg_free(freq[f])


@contextlib.contextmanager
def combo_outputs(L, rows: int = 2):
    """The same for the three outputs of an entry that returns one set of combinations -- the per-file arrays with one
    entry: take() -> (indices int32[rows, K], freq int32[K])."""
    with per_file_combo_outputs(L, 1, rows) as (outputs, take):
        yield outputs, lambda: take()[0]


@contextlib.contextmanager
def combo_matrix_outputs(L, n: int):
    """The five outputs of an entry that returns the combination matrix of n files (int32_t** indices_out, int64_t* k_out,
    int64_t** col_ptr_out, int32_t** rows_out, int32_t** freq_out).  `with ... as (outputs, take)`: pass `*outputs` to the
    call; after it, take() -> (indices int32[2, K], matrix int32[K, n] dense, as R's out.counts), fresh arrays that own their
    memory.  Leaving the block frees the four arrays, whatever happened inside."""
    idx, colptr, rows, freq, k = i32_p(), i64_p(), i32_p(), i32_p(), C.c_int64(0)

    def take():
        K = int(k.value)
        col = np.ctypeslib.as_array(colptr, shape=(n + 1,)).copy()
        nnz = int(col[n])
        indices = np.ctypeslib.as_array(idx, shape=(K, 2)).T.copy() if K else np.zeros((2, 0), dtype=np.int32)
        matrix = np.zeros((K, n), dtype=np.int32)
        if nnz:
            r = np.ctypeslib.as_array(rows, shape=(nnz,))
            matrix[r, np.repeat(np.arange(n), np.diff(col))] = np.ctypeslib.as_array(freq, shape=(nnz,))
        return indices, matrix
    try:
        yield (C.byref(idx), C.byref(k), C.byref(colptr), C.byref(rows), C.byref(freq)), take
    finally:
        for p in (idx, colptr, rows, freq):
            L.scg_free(p)


def decode_sequences(ptr, K: int, W: int):
    """K sequences of width W, NUL-terminated (stride W + 1) -> list[str], decoded as latin-1."""
    blob = C.string_at(ptr, K * (W + 1)) if K else b""
    return [blob[i * (W + 1): i * (W + 1) + W].decode("latin-1") for i in range(K)]
