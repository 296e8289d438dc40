#!/usr/bin/env python3
"""The paired single-barcode kernel (Plan.single_paired) against its yardstick: the single-end kernel on each mate alone.

    python tools/single_paired_bench.py --out profiles/single_paired_bench.json

Mate 1 is reads [0, n) of the config-2 workload (bench.py's headline: 150 bp, 100 k barcodes of 20 bases, <= 1 mismatch, both
strands), mate 2 reads [n, 2n); template, pool and budget are the workload's.  Six things are timed in one process, in turn,
round after round (the order rotating): the paired kernel in first and in best mode, and single_staged_kernel (Plan.single) on mate 1 and on
mate 2, in each of the two modes.  Every figure is the counting kernel alone, from the HIP events the plan records on the
launch stream around it (scg_plan_kernel_stats) -- the tally behind it is left out on both sides.  The yardstick of a
round and mode is the sum of its two single-mate times in that mode: the paired kernel stages and searches the same bytes
with the same walk (in first mode it skips mate 2's search for the lanes that hit on mate 1).  spread = the 5th to 95th
percentile of the rounds' sums.
"""
from __future__ import annotations

import argparse
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
    ap.add_argument("--pairs", type=int, default=50_000_000)
    ap.add_argument("--rounds", type=int, default=200, help="timed launches of each of the six kernels")
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()

    import torch
    import screencounter_amd as sc
    from screencounter_amd import synth
    assert torch.cuda.is_available(), "single_paired_bench.py needs a GPU"
    n = args.pairs
    w = synth.workload(2, n_reads=2 * n)
    dw = synth.DeviceWorkload(w, "cuda:0")
    mates = [dw.generate(n, first_read=0), dw.generate(n, first_read=n)]
    torch.cuda.synchronize()
    L = w.read_len

    def paired(use_first):
        return sc.Plan.single_paired(w.template, w.strand, w.pools[0], w.mismatches, use_first, device=0)

    def single(use_first):
        return sc.Plan.single(w.template, w.strand, w.pools[0], w.mismatches, use_first, device=0)

    plans = {"paired_first": paired(True), "paired_best": paired(False),
             "single_first_mate1": single(True), "single_first_mate2": single(True),
             "single_best_mate1": single(False), "single_best_mate2": single(False)}

    def launch(name):
        """One launch; the counting kernel's milliseconds."""
        plan = plans[name]
        plan.set_profiling(True)                       # (restarts the plan's event window)
        if name.startswith("paired"):
            plan.count_paired(mates[0], mates[1], fixed_len1=L, fixed_len2=L, n_pairs=n)
        else:
            plan.count(mates[0] if name.endswith("mate1") else mates[1], fixed_len=L, n_reads=n)
        ms, launches = plan.kernel_stats()
        assert launches == 1
        return ms

    for _ in range(args.warmup):
        for name in plans:
            launch(name)
    for plan in plans.values():
        plan.reset()
    times = {name: [] for name in plans}
    names = list(plans)
    for r in range(args.rounds):                       # (the order rotates, so that no kernel always follows the same one)
        for k in range(len(names)):
            name = names[(r + k) % len(names)]
            times[name].append(launch(name))
    counted = {}
    for name, plan in plans.items():
        counts, total = plan.read()
        counted[name] = {"mapped": int(counts.sum()), "total": int(total)}
        plan.close()

    bytes_per_pair = 2 * L
    result = {
        "tool": "tools/single_paired_bench.py", "device": torch.cuda.get_device_name(0), "workload": w.describe(),
        "pairs": n, "rounds": args.rounds, "warmup": args.warmup,
        "kernel_ms": {name: summary(xs) for name, xs in times.items()},
        "bytes_per_pair": bytes_per_pair,
        "counted": counted,
    }
    for mode in ("first", "best"):
        sums = [a + b for a, b in zip(times[f"single_{mode}_mate1"], times[f"single_{mode}_mate2"])]
        spread = percentile(sums, 0.95) - percentile(sums, 0.05)
        med = statistics.median(times["paired_" + mode])
        result[f"yardstick_{mode}_sum_of_single_mates"] = dict(summary(sums), spread_p05_p95_ms=round(spread, 4))
        result[f"paired_{mode}_vs_yardstick"] = {
            "ratio": round(med / statistics.median(sums), 4),
            "excess_ms": round(med - statistics.median(sums), 4),
            "within_spread": bool(med <= statistics.median(sums) + spread),
            "hbm_share_on_algorithmic_bytes": round(n * bytes_per_pair / (med * 1e-3) / 1e9 / HBM_PEAK_GBS, 4),
        }
    text = json.dumps(result, indent=1)
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
