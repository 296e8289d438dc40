#!/usr/bin/env python3
"""The assign kernel (Plan.assign / scg_assign_batch) against its yardstick: the counting kernel of the same build.

    SCG_TALLY=1 python tools/assign_bench.py --out profiles/assign_bench.json

One resident batch of the config-2 workload (bench.py's headline: 150 bp, 100 k barcodes of 20 bases, <= 1 mismatch, both
strands) goes, in one process and in turn, through single_staged_kernel writing the index stream of the tally (SCG_TALLY=1:
4 bytes per read) and through assign_staged_kernel of the same shape writing all five arrays (15 bytes per read).  Both
figures are the kernel alone, between device events on the launch stream: the plan's own events for the counting kernel
(scg_plan_kernel_stats; the tally kernel behind it is left out), events around the one launch of scg_assign_batch with
preallocated outputs for the other.  Each round times the two in alternating order.  The expectation is the ratio of the
algorithmic bytes per read, (150 + 15) / (150 + 4); spread = the 5th to 95th percentile of the per-round ratios.
"""
from __future__ import annotations

import argparse
import ctypes as C
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

HBM_PEAK_GBS = 8000.0


def percentile(xs, q):
    s = sorted(xs)
    return s[min(len(s) - 1, max(0, int(round(q * (len(s) - 1)))))]


def summary(xs):
    return {"median_ms": round(statistics.median(xs), 4), "min_ms": round(min(xs), 4), "max_ms": round(max(xs), 4),
            "p05_ms": round(percentile(xs, 0.05), 4), "p95_ms": round(percentile(xs, 0.95), 4)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reads", type=int, default=50_000_000)
    ap.add_argument("--rounds", type=int, default=200, help="timed launches of each kernel")
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if os.environ.get("SCG_TALLY") != "1":
        sys.exit("run with SCG_TALLY=1: the yardstick is the counting kernel writing the index stream")

    import torch
    import screencounter_amd as sc
    from screencounter_amd import _lib, synth
    assert torch.cuda.is_available(), "assign_bench.py needs a GPU"
    n = args.reads
    w = synth.workload(2, n_reads=n)
    reads = synth.DeviceWorkload(w, "cuda:0").generate(n)
    L = w.read_len
    out = [torch.empty(n, dtype=torch.int32 if k < 2 else torch.int8, device="cuda:0") for k in range(5)]
    torch.cuda.synchronize()
    lib = _lib.load()
    stream = torch.cuda.current_stream()
    result = {"tool": "tools/assign_bench.py", "device": torch.cuda.get_device_name(0), "workload": w.describe(), "reads": n,
              "rounds": args.rounds, "warmup": args.warmup, "bytes_per_read": {"count": L + 4, "assign": L + 15},
              "expected_ratio_of_algorithmic_bytes": round((L + 15) / (L + 4), 4)}
    for mode, use_first in (("first", True), ("best", False)):
        plan = sc.Plan.single(w.template, w.strand, w.pools[0], w.mismatches, use_first, device=0)

        def count():
            plan.set_profiling(True)                   # (restarts the plan's event window)
            plan.count(reads, fixed_len=L, n_reads=n)
            ms, launches = plan.kernel_stats()
            assert launches == 1
            return ms

        def assign():
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            err = _lib.errbuf()
            a.record(stream)
            _lib.check(lib.scg_assign_batch(plan._h, C.c_void_p(reads.data_ptr()), None, L, L, n, *(C.c_void_p(t.data_ptr()) for t in out),
                                            C.c_void_p(stream.cuda_stream), err, _lib.ERRCAP), err)
            b.record(stream)
            b.synchronize()
            return a.elapsed_time(b)

        for _ in range(args.warmup):
            count()
            assign()
        plan.reset()
        times = {"count": [], "assign": []}
        for r in range(args.rounds):                   # (the order alternates, so that neither kernel always follows the other)
            for name in (("count", "assign") if r % 2 == 0 else ("assign", "count")):
                times[name].append(count() if name == "count" else assign())
        counts, total = plan.read()
        index = out[0]
        assigned = int((index >= 0).sum().item())
        assert total == n * args.rounds and int(counts.astype("int64").sum()) == assigned * args.rounds, "the two kernels disagree on the reads matched"
        plan.close()
        ratios = [a / c for a, c in zip(times["assign"], times["count"])]
        spread = percentile(ratios, 0.95) - percentile(ratios, 0.05)
        ratio = statistics.median(times["assign"]) / statistics.median(times["count"])
        result[mode] = {
            "kernel_ms": {k: summary(v) for k, v in times.items()},
            "assigned_reads": assigned,
            "ratio_assign_over_count": round(ratio, 4),
            "ratio_spread_p05_p95": round(spread, 4),
            "above_expectation_by_more_than_the_spread": bool(ratio > (L + 15) / (L + 4) + spread),
            "hbm_share_on_algorithmic_bytes": {k: round(n * (L + (15 if k == "assign" else 4)) / (statistics.median(v) * 1e-3) / 1e9 / HBM_PEAK_GBS, 4)
                                               for k, v in times.items()},
        }
    text = json.dumps(result, indent=1)
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
