"""A plate of plain FASTQ files through scg_count_random_barcodes_files (every device of the call keeps one tally in HBM,
DESIGN.md §8.1) and through a loop of scg_count_random_barcodes (device search, host tally) over the same files, in one
process: wall times of both, and whether the two results are identical.

    python tools/random_files_rate.py --out profiles/random_files_rate.txt

Reads are made on the host from a seed: random bases with the construct ACGTAC + key + TTGCAG at offset 40, the key
drawn from one table of --keys 20-base keys shared by all files, a third of the reads reverse-complemented; the files are
written with synth.reads_to_fastq.  Each way is called --repeats times, alternating, after one untimed call of each (page
cache, window slots, code objects); the host clock is around calls that return only when their results are on the host.
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

READ_LEN = 150
LEFT, RIGHT, KEY_LEN, AT = b"ACGTAC", b"TTGCAG", 20, 40
TEMPLATE = LEFT.decode() + "-" * KEY_LEN + RIGHT.decode()


def make_reads(n, table, seed):
    rng = np.random.default_rng(seed)
    acgt = np.frombuffer(b"ACGT", dtype=np.uint8)
    comp = np.zeros(256, dtype=np.uint8)
    comp[acgt] = np.frombuffer(b"TGCA", dtype=np.uint8)
    reads = acgt[rng.integers(0, 4, (n, READ_LEN), dtype=np.uint8)]
    reads[:, AT:AT + len(LEFT)] = np.frombuffer(LEFT, dtype=np.uint8)
    reads[:, AT + len(LEFT):AT + len(LEFT) + KEY_LEN] = table[rng.integers(0, len(table), n)]
    reads[:, AT + len(LEFT) + KEY_LEN:AT + len(LEFT) + KEY_LEN + len(RIGHT)] = np.frombuffer(RIGHT, dtype=np.uint8)
    rev = rng.random(n) < 1 / 3
    reads[rev] = comp[reads[rev][:, ::-1]]
    return reads.reshape(-1)


def loop_of_one_file_calls(sc, paths, threads):
    """matrixOfRandomBarcodes as the reference builds it (R/countRandomBarcodes.R:85-92) over the one-file entry."""
    out = [sc.count_random_barcodes(p, TEMPLATE, 2, 0, True, threads) for p in paths]
    keys = sorted(set().union(*[o[0][0] for o in out]))
    row = {k: i for i, k in enumerate(keys)}
    matrix = np.zeros((len(keys), len(paths)), dtype=np.int32)
    for c, ((seqs, freq), _total) in enumerate(out):
        matrix[[row[s] for s in seqs], c] = freq
    return keys, matrix, np.array([o[1] for o in out], dtype=np.int32)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--files", type=int, default=8)
    ap.add_argument("--reads", type=int, default=2_000_000, help="reads per file")
    ap.add_argument("--keys", type=int, default=100_000)
    ap.add_argument("--threads", type=int, default=16)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()

    import torch
    import screencounter_amd as sc
    assert torch.cuda.is_available(), "random_files_rate.py needs a GPU"
    from screencounter_amd import synth

    table = np.frombuffer(b"ACGT", dtype=np.uint8)[np.random.default_rng(12345).integers(0, 4, (args.keys, KEY_LEN))]
    tmpdir = tempfile.mkdtemp(prefix="rfr")
    try:
        paths = []
        for f in range(args.files):
            paths.append(os.path.join(tmpdir, f"sample{f}.fastq"))
            synth.reads_to_fastq(paths[-1], make_reads(args.reads, table, 1000 + f), READ_LEN)
        size = sum(os.path.getsize(p) for p in paths)
        n_devices = min(sc.load().scg_device_count(), args.files) if not os.environ.get("SCG_DEVICES") else None
        lines = [f"# random_files_rate.py: {args.files} plain FASTQ files of {args.reads} reads of {READ_LEN} bp ({size / 1e9:.2f} GB in all, "
                 f"page cache warm), {args.keys} keys of {KEY_LEN} bases shared by all files, template {TEMPLATE} (strand both, "
                 f"0 mismatches, first match), {args.threads} host threads; {torch.cuda.get_device_name(0)}, "
                 f"devices of the many-files call: {n_devices if n_devices is not None else 'SCG_DEVICES=' + os.environ['SCG_DEVICES']}",
                 "# host clock around each call (both return with their results on the host; the loop includes building the union "
                 "and the matrix in Python, the many-files call building the dense matrix from its columns); one untimed call of "
                 "each first, then alternating"]
        many = lambda: sc.count_random_barcodes_files(paths, TEMPLATE, 2, 0, True, args.threads)      # noqa: E731
        loop = lambda: loop_of_one_file_calls(sc, paths, args.threads)                                 # noqa: E731
        got, ref = many(), loop()
        same = got[0] == ref[0] and np.array_equal(got[1], ref[1]) and np.array_equal(got[2], ref[2])
        t_many, t_loop = [], []
        for _ in range(args.repeats):
            t0 = time.perf_counter(); many(); t_many.append(time.perf_counter() - t0)                  # noqa: E702
            t0 = time.perf_counter(); loop(); t_loop.append(time.perf_counter() - t0)                  # noqa: E702
        n = args.files * args.reads
        for name, t in (("scg_count_random_barcodes_files (tally in HBM)", t_many), ("loop of scg_count_random_barcodes (host tally)", t_loop)):
            lines.append(f"{name:50s} {min(t) * 1e3:9.1f} ms  {n / min(t) / 1e6:7.1f} Mreads/s  (calls {' '.join(f'{x * 1e3:.1f}' for x in t)})")
        lines.append(f"K = {len(got[0])} rows, {int(got[1].sum())} of {int(got[2].sum())} reads counted; results identical: {same}")
    finally:
        shutil.rmtree(tmpdir, ignore_errors=True)
    print("\n".join(lines), flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")
    return 0 if same else 1


if __name__ == "__main__":
    sys.exit(main())
