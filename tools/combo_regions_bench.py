#!/usr/bin/env python3
"""The region-combination kernel (Plan.combo_regions) against its yardstick: combo_staged_kernel of the same build.

    python tools/combo_regions_bench.py --out profiles/combo_regions_bench.json

One resident batch of the config-3 workload (150 bp, 2 x 500 barcodes of 14 bases, <= 1 mismatch, both strands) goes, in one
process and in turn, through combo_staged_kernel (Plan.combo) and through combo_regions_staged_kernel at two regions
(Plan.combo_regions) in the same output mode: atomics on the replicated cells (SCG_TALLY=0: the new kernels write no index
stream, so the two-region kernel's tally mode is switched off for the comparison) and key streams (SCG_DENSE_CELLS=0).
Both figures are the kernel alone, between the plan's own device events on the launch stream (scg_plan_kernel_stats: the
fold, or the sort and run-length encode, behind it is left out).  Each round times the two in alternating order.  By
algorithmic bytes the two are equal (one read in, one cell or one 8-byte key out), so the expected ratio is 1; spread =
the 5th to 95th percentile of the per-round ratios.  Known differences of the new kernel: 64-bit key arithmetic (one
64-bit multiply-add per region), strides and eight descriptors in LDS, a loop over a run-time number of regions.

A three-region workload (3 x 500 pools of 14 bases, the same flanks, reads made here on the device) has no yardstick: it is
reported as reads per second and as a share of the HBM roofline on its algorithmic bytes.
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


def three_region_reads(torch, template, pools, n, L, seed, chunk=1 << 20):
    """n reads of L bases on the device: random bases, in 95 % of them the construct of one random barcode per pool at a
    random offset with 1 % substitutions, half of the reads reverse-complemented.  Made a chunk of reads at a time."""
    dev = "cuda:0"
    g = torch.Generator(device=dev)
    g.manual_seed(seed)
    letters = torch.tensor(list(b"ACGT"), dtype=torch.uint8, device=dev)
    comp = torch.arange(256, dtype=torch.uint8, device=dev)
    for x, y in zip(b"ACGT", b"TGCA"):
        comp[x] = y
    T = len(template)
    tables, starts, at = [], [], 0
    for pool in pools:
        a = template.index("-", at)
        tables.append(torch.tensor([list(s.encode()) for s in pool], dtype=torch.uint8, device=dev))
        starts.append(a)
        at = a + len(pool[0])
    constant = torch.tensor(list(template.encode()), dtype=torch.uint8, device=dev)
    out = torch.empty((n, L), dtype=torch.uint8, device=dev)
    for lo in range(0, n, chunk):
        m = min(chunk, n - lo)
        reads = letters[torch.randint(0, 4, (m, L), generator=g, device=dev)]
        construct = constant.repeat(m, 1)
        for table, a in zip(tables, starts):
            construct[:, a:a + table.shape[1]] = table[torch.randint(0, table.shape[0], (m,), generator=g, device=dev)]
        sub = torch.rand((m, T), generator=g, device=dev) < 0.01
        construct = torch.where(sub, letters[torch.randint(0, 4, (m, T), generator=g, device=dev)], construct)
        keep = torch.rand((m,), generator=g, device=dev) < 0.95
        off = torch.randint(0, L - T + 1, (m,), generator=g, device=dev)
        cols = off[:, None] + torch.arange(T, device=dev)[None, :]
        rows = torch.arange(m, device=dev)[:, None].expand(m, T)
        reads[rows[keep], cols[keep]] = construct[keep]
        flip = torch.rand((m,), generator=g, device=dev) < 0.5
        reads[flip] = comp[reads[flip].long()].flip(1)
        out[lo:lo + m] = reads
    return out.reshape(-1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reads", type=int, default=50_000_000)
    ap.add_argument("--reads3", type=int, default=10_000_000, help="reads of the three-region workload")
    ap.add_argument("--rounds", type=int, default=200, help="timed launches of each kernel")
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()

    import torch
    import screencounter_amd as sc
    from screencounter_amd import synth
    assert torch.cuda.is_available(), "combo_regions_bench.py needs a GPU"
    n = args.reads
    w = synth.workload(3, n_reads=n)
    reads = synth.DeviceWorkload(w, "cuda:0").generate(n)
    L = w.read_len
    torch.cuda.synchronize()
    result = {"tool": "tools/combo_regions_bench.py", "device": torch.cuda.get_device_name(0), "workload": w.describe(), "reads": n,
              "rounds": args.rounds, "warmup": args.warmup, "expected_ratio_of_algorithmic_bytes": 1.0,
              "known_differences": "64-bit mixed-radix key (one 64-bit multiply-add per region), strides and eight pool descriptors in LDS "
                                   "(896 bytes against 208), a loop over a run-time number of regions"}

    def timed(plan, data, count):
        plan.set_profiling(True)                       # (restarts the plan's event window)
        plan.count(data, fixed_len=L, n_reads=count)
        ms, launches = plan.kernel_stats()
        assert launches == 1
        return ms

    os.environ["SCG_TALLY"] = "0"
    for mode, dense_cells, out_bytes in (("dense cells (atomics)", None, 4), ("key stream", "0", 8)):
        if dense_cells is None:
            os.environ.pop("SCG_DENSE_CELLS", None)
        else:
            os.environ["SCG_DENSE_CELLS"] = dense_cells
        for use_first in (True, False):
            old = sc.Plan.combo(w.template, w.strand, w.pools[0], w.pools[1], w.mismatches, use_first, device=0)
            new = sc.Plan.combo_regions(w.template, w.strand, w.pools, w.mismatches, use_first, device=0)
            plans = {"combo": old, "combo_regions": new}
            for _ in range(args.warmup):
                for p in plans.values():
                    timed(p, reads, n)
            for p in plans.values():
                p.reset()
            times = {k: [] for k in plans}
            for r in range(args.rounds):               # (the order alternates, so that neither kernel always follows the other)
                for name in (("combo", "combo_regions") if r % 2 == 0 else ("combo_regions", "combo")):
                    times[name].append(timed(plans[name], reads, n))
            a, b = old.read_combinations(), new.read_combinations()
            assert a[2] == b[2] and (a[0] == b[0]).all() and (a[1] == b[1]).all(), "the two kernels disagree on the combinations counted"
            for p in plans.values():
                p.close()
            ratios = [x / y for x, y in zip(times["combo_regions"], times["combo"])]
            spread = percentile(ratios, 0.95) - percentile(ratios, 0.05)
            ratio = statistics.median(times["combo_regions"]) / statistics.median(times["combo"])
            result[f"{mode}, {'first' if use_first else 'best'}"] = {
                "kernel_ms": {k: summary(v) for k, v in times.items()},
                "counted_reads_per_launch": int(a[1].astype("int64").sum()) // args.rounds,
                "ratio_regions_over_combo": round(ratio, 4),
                "ratio_spread_p05_p95": round(spread, 4),
                "above_1_by_more_than_the_spread": bool(ratio > 1.0 + spread),
                "greads_per_s": {k: round(n / (statistics.median(v) * 1e-3) / 1e9, 3) for k, v in times.items()},
                "hbm_share_on_algorithmic_bytes": {k: round(n * (L + out_bytes) / (statistics.median(v) * 1e-3) / 1e9 / HBM_PEAK_GBS, 4) for k, v in times.items()},
            }
    # context: the two-region kernel in its default mode at this size (index stream; the tally behind it is not timed)
    os.environ.pop("SCG_TALLY", None)
    os.environ.pop("SCG_DENSE_CELLS", None)
    with sc.Plan.combo(w.template, w.strand, w.pools[0], w.pools[1], w.mismatches, True, device=0) as p:
        for _ in range(args.warmup):
            timed(p, reads, n)
        t = [timed(p, reads, n) for _ in range(args.rounds // 4)]
    result["combo in its default mode (index stream for the tally), first"] = {"kernel_ms": summary(t)}
    del reads
    torch.cuda.empty_cache()

    # three regions: no yardstick
    n3 = args.reads3
    t3 = synth.FLANK5[:12] + "-" * 14 + synth.FLANK5[12:] + "-" * 14 + synth.FLANK3[:12] + "-" * 14 + synth.FLANK3[12:]
    pools3 = [synth.random_library(500, 14, synth.BASE_SEED + 3 + 1000 * r) for r in range(3)]
    reads3 = three_region_reads(torch, t3, pools3, n3, L, 33)
    torch.cuda.synchronize()
    three = {"workload": f"{n3} reads x {L}bp, template of {len(t3)} bases, library 500 x 500 x 500 (1.25e8 combinations: key stream), <=1mm, both strands",
             "yardstick": "none: no other kernel of this project or of the reference counts three regions on a GPU"}
    for use_first in (True, False):
        with sc.Plan.combo_regions(t3, 2, pools3, 1, use_first, device=0) as p:
            assert p.num_counters == 0
            warm = [timed(p, reads3, n3) for _ in range(args.warmup)]
            p.reset()
            t = []
            for r in range(args.rounds):
                t.append(timed(p, reads3, n3))
                p.reset()                              # (the batch's runs are dropped, not merged on the host: millions of distinct keys)
            timed(p, reads3, n3)
            idx, freq, total = p.read_combinations()
            assert total == n3
        med = statistics.median(t)
        three["first" if use_first else "best"] = {
            "kernel_ms": summary(t), "slowest_launch": {"index": t.index(max(t)), "ms": round(max(t), 4)},
            "warmup_ms": [round(x, 4) for x in warm], "first_launches_ms": [round(x, 4) for x in t[:4]], "counted_reads_per_launch": int(freq.astype("int64").sum()), "distinct_combinations_per_launch": int(freq.size),
            "greads_per_s": round(n3 / (med * 1e-3) / 1e9, 3),
            "hbm_share_on_algorithmic_bytes": round(n3 * (L + 8) / (med * 1e-3) / 1e9 / HBM_PEAK_GBS, 4),
        }
    result["three regions"] = three
    text = json.dumps(result, indent=1)
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
