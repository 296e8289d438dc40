"""Config-scale parity: the HIP path on the ACTUAL libraries and read streams of BASELINE.json's configurations
(synth.workload(c): 100 k-barcode library with its 256 Ki-slot tables and chains, 2 x 500 pools, 50 k pairs, the six
pairs-of-quarters tables of <= 2 mismatches), against real kaori's counts on the same reads.

kaori's outputs are committed in tests/golden/config_scale_kaori.json (oracle/gen_golden.py::config_scale_fixture) as
SHA-256 digests of its count vectors with their totals, sums and numbers of non-zero entries, next to a digest of every
read stream they were computed on, so that no checker is needed where the tests run.  The parity streams have >= 2^20
reads, large enough for the index-stream + tally path to be the one that runs.

Both the HBM-resident batch entry (scg_count_batch*) and the file-level entry points (FASTQ -> pinned staging ->
counts) are checked.  The device generator is checked byte for byte against its numpy restatement on the way.
Reference: handlers/SingleBarcodeSingleEnd.hpp:93-104, CombinatorialBarcodesSingleEnd.hpp:149-258,
DualBarcodesPairedEnd.hpp:258-347."""
import hashlib
import json
import os

import numpy as np
import pytest

from tests.test_config1_fixture import load_fixture

pytestmark = pytest.mark.gpu

FIXTURE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "config_scale_kaori.json")
PARITY_READS = {2: (1 << 20) + 4321, 3: (1 << 20) + 4321, 4: (1 << 20) + 999, 5: (1 << 20) + 4321}
OPTION_READS = (1 << 18) + 77


def dense_combo(idx, freq, n1, size):
    cells = np.zeros(size, dtype=np.int64)
    if freq.size:
        cells[idx[0].astype(np.int64) * n1 + idx[1]] = freq
    return cells


def parity_key(config):
    return f"parity_{config}"


def option_key(config, use_first, strand, randomized, mismatches):
    return f"options_{config}_{int(use_first)}_{strand}_{int(randomized)}_{'w' if mismatches is None else mismatches}"


def stream_digest(host):
    h = hashlib.sha256()
    for arr in host:
        h.update(np.ascontiguousarray(arr).tobytes())
    return h.hexdigest()


def count_record(counts, total):
    """What the fixture keeps of a (counts, total) result: the digest of the counts as little-endian int64 decides equality,
    the sum and the number of non-zero entries say how far apart two results are."""
    c = np.ascontiguousarray(np.asarray(counts, dtype="<i8"))
    return {"total": int(total), "mapped": int(c.sum()), "nonzero": int(np.count_nonzero(c)),
            "counts_sha256": hashlib.sha256(c.tobytes()).hexdigest()}


def expected(key, host):
    """kaori's count record for fixture case `key`, after checking that `host` (the mates' reads) is the stream kaori
    was run on."""
    with open(FIXTURE) as f:
        rec = json.load(f)["cases"][key]
    assert stream_digest(host) == rec["reads_sha256"], f"{key}: the read stream is no longer the one kaori was run on (oracle/gen_golden.py configs)"
    return {k: rec[k] for k in ("total", "mapped", "nonzero", "counts_sha256")}


def assert_counts(counts, total, exp, what):
    got = count_record(counts, total)
    assert got == exp, f"{what} differs from kaori: {got} vs {exp}"


@pytest.mark.parametrize("config", [2, 3, 4, 5])
def test_config_scale_parity(sc, gpu, tmp_path, config):
    from screencounter_amd import synth
    n = PARITY_READS[config]                        # >= 2^20: tally mode is what runs
    w = synth.workload(config, n_reads=n)
    L = w.read_len
    dw = synth.DeviceWorkload(w, gpu)
    mates = [dw.generate(n, mate=0)]
    if w.entry == "dual":
        mates.append(dw.generate(n, mate=1))
    host = [m.cpu().numpy() for m in mates]
    # the device generator against its numpy restatement (first and a late slice)
    k = 30_000
    for m in range(len(mates)):
        assert np.array_equal(host[m][: k * L], synth.generate_host(w, k, first_read=0, mate=m))
        assert np.array_equal(host[m][(n - 1000) * L:], synth.generate_host(w, 1000, first_read=n - 1000, mate=m))
    exp = expected(parity_key(config), host)
    with dw.plan() as plan:
        if w.entry == "dual":
            plan.count_paired(mates[0], mates[1], fixed_len1=L, fixed_len2=L, n_pairs=n)
        else:
            plan.count(mates[0], fixed_len=L, n_reads=n)
        got, total = plan.read()
    assert total == exp["total"] == n
    assert_counts(got, total, exp, f"HIP path on config {config}")
    assert exp["mapped"] > 0.8 * n
    # the same reads through the file-level entry points (parallel FASTQ stager -> pinned -> H2D -> kernels)
    paths = []
    for m, arr in enumerate(host):
        paths.append(str(tmp_path / f"cfg{config}_{m}.fastq"))
        synth.reads_to_fastq(paths[-1], arr, L)
    if w.entry == "single":
        c, t = sc.count_single_barcodes(paths[0], w.template, w.strand, w.pools[0], w.mismatches, w.use_first, 4)
        c = c.astype(np.int64)
    elif w.entry == "combo":
        idx, freq, t = sc.count_combo_barcodes_single(paths[0], w.template, w.strand, [w.pools[0], w.pools[1]], w.mismatches, w.use_first, 4)
        c = dense_combo(idx, freq, len(w.pools[1]), len(w.pools[0]) * len(w.pools[1]))
    else:
        c, t = sc.count_dual_barcodes(paths[0], w.template, False, w.mismatches, w.pools[0], paths[1], w.template2, False, w.mismatches,
                                      w.pools[1], False, w.use_first, False, 4)
        c = c.astype(np.int64)
    assert_counts(c, t, exp, f"file-level entry on config {config}")


def test_config1_fixture_gpu(sc, gpu):
    """Config 1 on the HIP path against the committed kaori fixture (no checker needed on the box)."""
    from screencounter_amd import synth
    fx = load_fixture()
    w = synth.workload(1)
    dw = synth.DeviceWorkload(w, gpu)
    reads = dw.generate(w.n_reads)
    assert hashlib.sha256(reads.cpu().numpy().tobytes()).hexdigest() == fx["reads_sha256"]
    with dw.plan() as plan:
        plan.count(reads, fixed_len=w.read_len, n_reads=w.n_reads)
        got, total = plan.read()
    assert total == fx["expect"]["total"]
    assert got.tolist() == fx["expect"]["counts"]


def option_cases():
    cases = []
    for config in (2, 3, 5):
        for use_first in (True, False):
            for strand in (0, 1, 2):
                if (use_first, strand) == (True, 2):
                    continue                                  # the configuration's own option point: test_config_scale_parity
                cases.append((config, use_first, strand, False, None))
    for use_first in (True, False):
        for randomized in (False, True):
            if (use_first, randomized) == (True, False):
                continue
            cases.append((4, use_first, 0, randomized, None))
    for use_first in (True, False):
        cases.append((3, use_first, 2, False, 2))             # combinations with a budget of 2: the six pairs-of-quarters tables per pool
        cases.append((2, use_first, 2, False, 0))             # exact matching: one table, no walk
    return cases


@pytest.mark.parametrize("config,use_first,strand,randomized,mismatches", option_cases())
def test_config_scale_options(sc, gpu, config, use_first, strand, randomized, mismatches):
    """The other option points of every entry -- find.best = TRUE (search_best's tie logic over the 100 k-entry index,
    SimpleSingleMatch.hpp:259-306), strand = original / reverse, randomized = TRUE (DualBarcodesPairedEnd.hpp:353-371;
    config 4's pools are >= 3 apart, so the reference's cache-order hazard, SURVEY.md A.7, cannot occur) -- on 2^18 reads of
    the configuration's own stream and library, against real kaori."""
    from screencounter_amd import synth
    from screencounter_amd.engine import Plan
    n = OPTION_READS
    w = synth.workload(config, n_reads=n)
    L = w.read_len
    dw = synth.DeviceWorkload(w, gpu)
    mates = [dw.generate(n, mate=0)]
    if w.entry == "dual":
        mates.append(dw.generate(n, mate=1))
    if mismatches is not None:
        w.mismatches = mismatches                            # (the stream is the configuration's; only the budget differs)
    exp = expected(option_key(config, use_first, strand, randomized, mismatches), [t.cpu().numpy() for t in mates])
    dev = gpu.index if gpu.index is not None else 0
    if w.entry == "single":
        plan = Plan.single(w.template, strand, w.pools[0], w.mismatches, use_first, device=dev)
    elif w.entry == "combo":
        plan = Plan.combo(w.template, strand, w.pools[0], w.pools[1], w.mismatches, use_first, device=dev)
    else:
        plan = Plan.dual(w.template, False, w.mismatches, w.pools[0], w.template2, False, w.mismatches, w.pools[1],
                         randomized=randomized, use_first=use_first, device=dev)
    with plan:
        if w.entry == "dual":
            plan.count_paired(mates[0], mates[1], fixed_len1=L, fixed_len2=L, n_pairs=n)
        else:
            plan.count(mates[0], fixed_len=L, n_reads=n)
        got, total = plan.read()
    assert total == exp["total"] == n
    assert_counts(got, total, exp, f"HIP path on config {config}, use_first={use_first}, strand={strand}, randomized={randomized}")
    assert exp["mapped"] > (0.3 if (strand != 2 and w.entry != "dual") or mismatches == 0 else 0.7) * n
