"""Rates of random-barcode plans (Plan.random): count() and read_random() timed apart with HIP events on device-resident
150 bp reads, for 10^3, 10^6 and ~10^8 (all distinct) 20-base keys; the read-out of 10^7 distinct keys; and the file entry
point (scg_count_random_barcodes, host tally) on a plain FASTQ of 10 M of the same reads.

    python tools/random_plan_rate.py --out profiles/random_plan_rate.txt

Reads are made on the device from a seed: random bases with the construct ACGTAC + key + TTGCAG at offset 40, the key
drawn from a table of K keys (or fresh per read for "distinct"), a third of the reads reverse-complemented.
"""
from __future__ import annotations

import argparse
import os
import statistics
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


def make_batch(torch, n, n_keys, seed, device):
    """n reads of READ_LEN bytes (uint8, flat) on the device; n_keys = 0 gives every read a fresh key."""
    g = torch.Generator(device=device)
    g.manual_seed(seed)
    acgt = torch.tensor(list(b"ACGT"), dtype=torch.uint8, device=device)
    comp = torch.zeros(256, dtype=torch.uint8, device=device)
    comp[torch.tensor(list(b"ACGT"), device=device).long()] = torch.tensor(list(b"TGCA"), dtype=torch.uint8, device=device)
    reads = acgt[torch.randint(0, 4, (n, READ_LEN), generator=g, device=device)]
    reads[:, AT:AT + len(LEFT)] = torch.tensor(list(LEFT), dtype=torch.uint8, device=device)
    reads[:, AT + len(LEFT) + KEY_LEN:AT + len(LEFT) + KEY_LEN + len(RIGHT)] = torch.tensor(list(RIGHT), dtype=torch.uint8, device=device)
    if n_keys:
        kg = torch.Generator(device=device)
        kg.manual_seed(12345)
        table = acgt[torch.randint(0, 4, (n_keys, KEY_LEN), generator=kg, device=device)]
        reads[:, AT + len(LEFT):AT + len(LEFT) + KEY_LEN] = table[torch.randint(0, n_keys, (n,), generator=g, device=device)]
    rev = torch.rand(n, generator=g, device=device) < 1 / 3
    reads[rev] = comp[reads[rev].flip(1).long()]
    return reads.reshape(-1).contiguous()


def timed_count(torch, plan, batches, n_per):
    start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    start.record()
    for b in batches:
        plan.count(b, fixed_len=READ_LEN, n_reads=n_per)
    stop.record()
    torch.cuda.synchronize()
    return start.elapsed_time(stop)


def timed_read(torch, plan):
    """(ms of scg_plan_read_random alone, ms of Plan.read_random incl. the Python list of str, K, total)."""
    import ctypes as C
    from screencounter_amd import _lib
    torch.cuda.synchronize()
    seq_p, freq_p = C.c_void_p(), _lib.i32_p()
    k, vlen, total = C.c_int64(0), C.c_int32(0), C.c_int64(0)
    err = _lib.errbuf()
    stream = C.c_void_p(int(torch.cuda.current_stream().cuda_stream))
    t0 = time.perf_counter()
    _lib.check(plan._lib.scg_plan_read_random(plan._h, C.byref(seq_p), C.byref(freq_p), C.byref(k), C.byref(vlen), C.byref(total),
                                              stream, err, _lib.ERRCAP), err)
    c_ms = (time.perf_counter() - t0) * 1e3
    plan._lib.scg_free(seq_p)
    plan._lib.scg_free(freq_p)
    t0 = time.perf_counter()
    (seqs, freq), total = plan.read_random()
    py_ms = (time.perf_counter() - t0) * 1e3
    return c_ms, py_ms, len(seqs), total


def write_fastq(torch, path, batch, n):
    rows = batch[: n * READ_LEN].view(n, READ_LEN).cpu().numpy()
    rec = np.empty((n, 3 + READ_LEN + 3 + READ_LEN + 1), dtype=np.uint8)
    rec[:, 0:3] = np.frombuffer(b"@r\n", dtype=np.uint8)
    rec[:, 3:3 + READ_LEN] = rows
    rec[:, 3 + READ_LEN:6 + READ_LEN] = np.frombuffer(b"\n+\n", dtype=np.uint8)
    rec[:, 6 + READ_LEN:6 + 2 * READ_LEN] = ord("I")
    rec[:, -1] = ord("\n")
    rec.tofile(path)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reads", type=int, default=100_000_000, help="reads per key distribution")
    ap.add_argument("--batch", type=int, default=10_000_000)
    ap.add_argument("--repeats", type=int, default=2)
    ap.add_argument("--fastq-reads", type=int, default=10_000_000)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()

    import torch
    import screencounter_amd as sc
    assert torch.cuda.is_available(), "random_plan_rate.py needs a GPU"
    dev = torch.device("cuda:0")
    lines = [f"# random_plan_rate.py: {args.reads} reads of {READ_LEN} bp per distribution, batches of {args.batch}, "
             f"template {TEMPLATE} (strand both, 0 mismatches, first match); {torch.cuda.get_device_name(0)}",
             "# count(): HIP events around all batches (table growth included), median of repeats on a fresh plan; "
             "read-out: host clock around scg_plan_read_random (synchronises; compaction, device sort + decode, copies, host merge) "
             "and around Plan.read_random (the same + building the Python list of str)"]

    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")

    def emit(s):
        print(s, flush=True)
        lines.append(s)
        if args.out:                    # line by line, so that a cut-short run keeps what it measured
            with open(args.out, "a") as f:
                f.write(s + "\n")

    n_batches = args.reads // args.batch
    for label, n_keys in (("1e3 keys", 1000), ("1e6 keys", 1_000_000), ("distinct", 0)):
        batches = [make_batch(torch, args.batch, n_keys, 1000 * n_keys + i, dev) for i in range(n_batches)]
        # warm-up: one batch on a throwaway plan (module load, first launches)
        with sc.Plan.random(TEMPLATE, 2) as plan:
            plan.count(batches[0], fixed_len=READ_LEN, n_reads=args.batch)
            plan.read_random()
        counts, c_out, py_out = [], [], []
        for _ in range(args.repeats):
            with sc.Plan.random(TEMPLATE, 2) as plan:
                counts.append(timed_count(torch, plan, batches, args.batch))
                c_ms, py_ms, k, total = timed_read(torch, plan)
                c_out.append(c_ms)
                py_out.append(py_ms)
        c = statistics.median(counts)
        emit(f"{label:10s} count {c:9.1f} ms  {n_batches * args.batch / c / 1e3:8.1f} Mreads/s  "
             f"(repeats {' '.join(f'{x:.1f}' for x in counts)})   read-out C {statistics.median(c_out):8.1f} ms, Python {statistics.median(py_out):8.1f} ms "
             f"for K={k}  total={total}")
        del batches
        torch.cuda.empty_cache()

    # read-out of 10^7 distinct keys
    batch = make_batch(torch, 10_000_000, 0, 777, dev)
    with sc.Plan.random(TEMPLATE, 2) as plan:
        plan.count(batch, fixed_len=READ_LEN, n_reads=10_000_000)
        outs = [timed_read(torch, plan) for _ in range(args.repeats)]
    emit(f"read-out of K={outs[0][2]} distinct keys: C {statistics.median(o[0] for o in outs):.1f} ms "
         f"(repeats {' '.join(f'{o[0]:.1f}' for o in outs)}), Python {statistics.median(o[1] for o in outs):.1f} ms")
    del batch
    torch.cuda.empty_cache()

    # the file entry (host tally) against the plan on the same 10 M reads (10^6 keys)
    n = args.fastq_reads
    batch = make_batch(torch, n, 1_000_000, 4242, dev)
    with sc.Plan.random(TEMPLATE, 2) as plan:
        c = timed_count(torch, plan, [batch], n)
        r, rp, k, total = timed_read(torch, plan)
        (pseqs, pfreq), _ = plan.read_random()
    emit(f"plan, {n} reads, 1e6 keys: count {c:.1f} ms + read-out C {r:.1f} ms, Python {rp:.1f} ms  (K={k})")
    tmpdir = tempfile.mkdtemp(prefix="rpr")
    path = os.path.join(tmpdir, "reads.fastq")
    try:
        write_fastq(torch, path, batch, n)
        del batch
        walls = []
        for _ in range(2):
            t0 = time.perf_counter()
            (fseqs, ffreq), ftotal = sc.count_random_barcodes(path, TEMPLATE, 2, 0, True, 16)
            walls.append(time.perf_counter() - t0)
        same = fseqs == pseqs and np.array_equal(ffreq, pfreq) and ftotal == total
        emit(f"file entry scg_count_random_barcodes, plain FASTQ of {n} reads ({os.path.getsize(path) / 1e9:.2f} GB, page cache warm), "
             f"16 host threads: {min(walls) * 1e3:.1f} ms wall (calls {' '.join(f'{w * 1e3:.1f}' for w in walls)}); "
             f"same result as the plan: {same}")
    finally:
        if os.path.exists(path):
            os.remove(path)
        os.rmdir(tmpdir)


if __name__ == "__main__":
    main()
