"""screencounter_amd -- MI355X-native barcode counting engine behind screenCounter's hot path.

Package contents (only what the path needs):
  csrc/      HIP kernels (gfx950) + host runtime + the C ABI of include/scg.h -> libscg.so
  _lib.py    ctypes binding of libscg.so (fails loudly when the library is missing)
  engine.py  Plan objects over device-resident read batches
  api.py     mirror of the reference's Rcpp-level entry points for this path (same names, arguments, results)
  synth.py   synthetic workloads of SURVEY.md section 8(d) (device-side generator)
  parallel.py  read-sharded multi-GPU driver (torch.distributed over RCCL)
"""
from ._lib import ScgError, load, prepare_pool  # noqa: F401
from .api import (  # noqa: F401
    count_single_barcodes, count_combo_barcodes_single, count_dual_barcodes, count_combo_barcodes_paired,
    count_single_barcodes_files, count_combo_barcodes_single_files, count_dual_barcodes_files, count_dual_barcodes_single_end,
    count_dual_barcodes_diagnostics_files, count_dual_barcodes_single_end_files, count_dual_barcodes_single_end_diagnostics_files,
    count_combo_barcodes_paired_files, count_single_barcodes_paired, count_single_barcodes_paired_files, count_random_barcodes, count_random_barcodes_files, match_barcodes, parse_fastq,
    assign_single_barcodes, count_combo_barcodes_regions, count_combo_barcodes_regions_files,
    combine_combinations, count_combo_barcodes_single_matrix, count_combo_barcodes_paired_matrix, combo_compact_device,
)
from .engine import Assignment, Plan, combo_compact, upload_reads  # noqa: F401

__version__ = "0.3.0"
