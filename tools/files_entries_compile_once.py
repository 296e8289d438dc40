"""What compiling once saves: matrixOfDualBarcodes(include.invalid=TRUE)-shaped input -- 16 small pairs of files against
config 4's library of 50 000 pairs -- counted on one device two ways:

  files   one call of scg_count_dual_barcodes_diagnostics_files (template and pools compiled once, one plan for all files);
  loop    one call of scg_count_dual_barcodes_diagnostics per pair of files (compiled and uploaded per file), which is all a
          build without the many-files entry offers.

    tools/ab_build.sh <parent revision> parent
    python tools/files_entries_compile_once.py --mode files --out profiles/files_entries_compile_once.txt
    python tools/files_entries_compile_once.py --mode loop --lib tools/ab/parent.so --out profiles/files_entries_compile_once.txt

Each mode runs in its own process (--lib selects the build before the library is loaded), warms up on one pair of files,
then times `--repeats` passes over all of them; the pools are marshalled once (prepare_pool), as R hands its CHARSXPs over
without a copy.  Both modes must return the same results; a digest of them is printed for comparison.
"""
from __future__ import annotations

import argparse
import hashlib
import os
import random
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

BASES = "ACGT"


def write_files(w, root, n_files, n_pairs, seed):
    """n_files pairs of plain FASTQ files of n_pairs read pairs: 85 % valid pairs, 10 % invalid ones, 5 % junk."""
    rng = random.Random(seed)
    pool1, pool2 = w.pools
    t1, t2 = w.template, w.template2

    def fill(t, barcode):
        return t[:t.index("-")] + barcode + t[t.rindex("-") + 1:]

    def pad(s):
        left = rng.randrange(0, w.read_len - len(s) + 1)
        return "".join(rng.choices(BASES, k=left)) + s + "".join(rng.choices(BASES, k=w.read_len - len(s) - left))

    paths = []
    for f in range(n_files):
        p1, p2 = os.path.join(root, f"s{f}_1.fastq"), os.path.join(root, f"s{f}_2.fastq")
        with open(p1, "w") as o1, open(p2, "w") as o2:
            for i in range(n_pairs):
                u = rng.random()
                if u < 0.85:
                    k = rng.randrange(len(pool1))
                    a, b = pad(fill(t1, pool1[k])), pad(fill(t2, pool2[k]))
                elif u < 0.95:
                    a, b = pad(fill(t1, rng.choice(pool1))), pad(fill(t2, rng.choice(pool2)))
                else:
                    a, b = pad(""), pad("")
                o1.write(f"@r{i}\n{a}\n+\n{'I' * len(a)}\n")
                o2.write(f"@r{i}\n{b}\n+\n{'I' * len(b)}\n")
        paths.append((p1, p2))
    return paths


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--mode", choices=["files", "loop"], required=True)
    ap.add_argument("--lib", default=None, help="another build of libscg.so (tools/ab_build.sh), for --mode loop on the parent revision")
    ap.add_argument("--files", type=int, default=16)
    ap.add_argument("--pairs", type=int, default=2000, help="read pairs per file")
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--out", default=None, help="append the result lines to this file")
    args = ap.parse_args()
    if args.lib:
        os.environ["SCG_LIB"] = os.path.abspath(args.lib)
    os.environ["SCG_DEVICES"] = "0"                       # one device, both ways
    import screencounter_amd as sc
    from screencounter_amd import synth

    w = synth.workload(4)
    pool1, pool2 = sc.prepare_pool(w.pools[0]), sc.prepare_pool(w.pools[1])
    common1 = (w.template, False, w.mismatches, pool1)
    common2 = (w.template2, False, w.mismatches, pool2)

    def digest(per_file):
        h = hashlib.sha256()
        for counts, idx, freq, total, b1, b2 in per_file:
            h.update(counts.tobytes() + idx.tobytes() + freq.tobytes() + repr((total, b1, b2)).encode())
        return h.hexdigest()[:16]

    def run_files(paths):
        mat, inv, tot, b1, b2 = sc.count_dual_barcodes_diagnostics_files([a for a, _ in paths], *common1, [b for _, b in paths], *common2,
                                                                        False, True, 1, [0])
        return [(mat[:, f].copy(), inv[f][0], inv[f][1], tot[f], b1[f], b2[f]) for f in range(len(paths))]

    def run_loop(paths):
        out = []
        for a, b in paths:
            counts, (idx, freq), total, b1, b2 = sc.count_dual_barcodes(a, *common1, b, *common2, False, True, True, 1)
            out.append((counts, idx, freq, total, b1, b2))
        return out

    run = run_files if args.mode == "files" else run_loop
    with tempfile.TemporaryDirectory() as root:
        paths = write_files(w, root, args.files, args.pairs, seed=4)
        run(paths[:1])                                     # HIP start-up, code objects, pinned buffers
        times, result = [], None
        for _ in range(args.repeats):
            t0 = time.perf_counter()
            result = run(paths)
            times.append(time.perf_counter() - t0)
    total_pairs = sum(r[3] for r in result)
    line = (f"mode={args.mode} lib={args.lib or 'this build'} files={args.files} pairs_per_file={args.pairs} library={len(pool1)} pairs "
            f"device=0 wall_ms min={min(times) * 1e3:.1f} median={sorted(times)[len(times) // 2] * 1e3:.1f} max={max(times) * 1e3:.1f} "
            f"per_file_ms={min(times) * 1e3 / args.files:.1f} counted={total_pairs} digest={digest(result)}")
    print(line)
    if args.out:
        with open(args.out, "a") as f:
            f.write("# python " + " ".join(sys.argv) + "\n" + line + "\n")


if __name__ == "__main__":
    main()
