"""A plate of plain FASTQ files through scg_count_combo_barcodes_single_files (per-file lists; a dense histogram is copied
to the host whole and scanned there, and the merge is left to the caller) and through scg_count_combo_barcodes_single_matrix
(the histogram compacted on the device, the files' lists merged there: csrc/scg_combine.hip) in one process: wall times of
both, and whether the matrix is combineComboCounts of the per-file lists.

    python tools/combo_matrix_rate.py --out profiles/combo_matrix_rate.txt

Two plates, on tmpfs where there is one: pools of 2 x 500 barcodes, and of 8192 x 8192 -- 2^26 cells, the default dense
limit.  Reads are made on the host from a seed: random bases with the construct ACGTAC + first + GGTACA + second + TTGCAG
at offset 30, both barcodes drawn uniformly, a third of the reads reverse-complemented; the files are written with
synth.reads_to_fastq.  Each entry is called --repeats times, alternating, after one untimed call of each (page cache,
window slots, code objects); the host clock is around calls that return only when their results are on the host.  The
files entry's time leaves the merge undone; the matrix entry's includes it.
"""
from __future__ import annotations

import argparse
import os
import shutil
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

READ_LEN, AT, BARCODE = 150, 30, 12
LEFT, MID, RIGHT = b"ACGTAC", b"GGTACA", b"TTGCAG"
TEMPLATE = LEFT.decode() + "-" * BARCODE + MID.decode() + "-" * BARCODE + RIGHT.decode()
ACGT = np.frombuffer(b"ACGT", dtype=np.uint8)


def make_pool(n, seed):
    """n distinct barcodes of BARCODE bases as a uint8 [n, BARCODE] array."""
    values = np.random.default_rng(seed).choice(4**BARCODE, size=n, replace=False)
    return ACGT[(values[:, None] >> (2 * np.arange(BARCODE))) & 3]


def make_reads(n, pools, seed):
    rng = np.random.default_rng(seed)
    comp = np.zeros(256, dtype=np.uint8)
    comp[ACGT] = np.frombuffer(b"TGCA", dtype=np.uint8)
    reads = ACGT[rng.integers(0, 4, (n, READ_LEN), dtype=np.uint8)]
    at = AT
    for piece in (LEFT, pools[0], MID, pools[1], RIGHT):
        if isinstance(piece, bytes):
            reads[:, at:at + len(piece)] = np.frombuffer(piece, dtype=np.uint8)
            at += len(piece)
        else:
            reads[:, at:at + BARCODE] = piece[rng.integers(0, len(piece), n)]
            at += BARCODE
    rev = rng.random(n) < 1 / 3
    reads[rev] = comp[reads[rev][:, ::-1]]
    return reads.reshape(-1)


def combine(per_file):
    """combineComboCounts (R/combineComboCounts.R:31-57) of per-file (indices, freq, total) in numpy."""
    keys = [(i[0].astype(np.int64) << 32) | i[1] for i, _f, _t in per_file]
    union = np.unique(np.concatenate(keys))
    matrix = np.zeros((len(union), len(per_file)), dtype=np.int32)
    for c, (k, (_i, freq, _t)) in enumerate(zip(keys, per_file)):
        matrix[np.searchsorted(union, k), c] = freq
    return np.stack([union >> 32, union & 0xFFFFFFFF]).astype(np.int32), matrix


def spread(times):
    t = np.asarray(times) * 1e3
    return f"median {np.median(t):9.1f} ms, 5th-95th percentile {np.percentile(t, 5):9.1f} .. {np.percentile(t, 95):9.1f} ms"


def run_plate(sc, tmpdir, n0, n1, args, lines):
    pools = [make_pool(n0, 11), make_pool(n1, 22)]
    names = [[bytes(row).decode() for row in p] for p in pools]
    from screencounter_amd import synth
    paths = []
    for f in range(args.files):
        paths.append(os.path.join(tmpdir, f"sample_{n0}x{n1}_{f}.fastq"))
        synth.reads_to_fastq(paths[-1], make_reads(args.reads, pools, 1000 * n1 + f), READ_LEN)
    size = sum(os.path.getsize(p) for p in paths)
    prepared = [sc.prepare_pool(names[0]), sc.prepare_pool(names[1])]
    files = lambda: sc.count_combo_barcodes_single_files(paths, TEMPLATE, 2, prepared, 0, True, args.threads)      # noqa: E731
    matrix = lambda: sc.count_combo_barcodes_single_matrix(paths, TEMPLATE, 2, prepared, 0, True, args.threads)    # noqa: E731
    per_file, got = files(), matrix()
    exp_idx, exp_matrix = combine(per_file)
    same = (np.array_equal(got[0], exp_idx) and np.array_equal(got[1], exp_matrix) and got[2].tolist() == [t for _i, _f, t in per_file])
    t_files, t_matrix = [], []
    for _ in range(args.repeats):
        t0 = time.perf_counter(); files(); t_files.append(time.perf_counter() - t0)                                # noqa: E702
        t0 = time.perf_counter(); matrix(); t_matrix.append(time.perf_counter() - t0)                              # noqa: E702
    lines.append(f"## pools {n0} x {n1} = {n0 * n1} cells ({n0 * n1 * 4 / 1e6:.1f} MB of cells per file); {args.files} files of {args.reads} reads "
                 f"({size / 1e9:.2f} GB in all); K_f = {' '.join(str(len(f)) for _i, f, _t in per_file)}; K = {got[1].shape[0]}")
    for name, t in (("scg_count_combo_barcodes_single_files  (merge not done)", t_files), ("scg_count_combo_barcodes_single_matrix (merge included)", t_matrix)):
        lines.append(f"{name:58s} {spread(t)}  (calls {' '.join(f'{x * 1e3:.1f}' for x in t)})")
    d = (np.median(t_matrix) - np.median(t_files)) * 1e3
    lines.append(f"matrix median - files median = {d:+.1f} ms; matrix is combineComboCounts of the files entry's lists: {same}")
    for p in paths:
        os.remove(p)
    return same


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--files", type=int, default=8)
    ap.add_argument("--reads", type=int, default=250_000, help="reads per file")
    ap.add_argument("--threads", type=int, default=16)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if args.repeats < 5:
        ap.error("--repeats: at least 5 timed calls of each entry")

    import torch
    import screencounter_amd as sc
    assert torch.cuda.is_available(), "combo_matrix_rate.py needs a GPU"

    tmpdir = tempfile.mkdtemp(prefix="cmr", dir="/dev/shm" if os.path.isdir("/dev/shm") else None)
    try:
        n_devices = min(sc.load().scg_device_count(), args.files) if not os.environ.get("SCG_DEVICES") else None
        lines = [f"# combo_matrix_rate.py: plain FASTQ files of {READ_LEN} bp reads in {tmpdir.rsplit('/', 1)[0]} (page cache warm), template {TEMPLATE} "
                 f"(strand both, 0 mismatches, first match), {args.threads} host threads; {torch.cuda.get_device_name(0)}, "
                 f"devices of the calls: {n_devices if n_devices is not None else 'SCG_DEVICES=' + os.environ['SCG_DEVICES']}",
                 "# host clock around each call (both return with their results on the host; the matrix entry's time includes building "
                 "the dense K x files matrix from its columns in Python); one untimed call of each first, then alternating, "
                 f"{args.repeats} timed calls each"]
        ok = True
        for n0, n1 in ((2, 500), (8192, 8192)):
            ok = run_plate(sc, tmpdir, n0, n1, args, lines) and ok
    finally:
        shutil.rmtree(tmpdir, ignore_errors=True)
    print("\n".join(lines), flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
