"""The late-flaw files of test_gpu_late_fallback.py where no GPU is present: the file-level parse (the multi-threaded reader
first, the sequential reader when it finds the file unusual, scg_api.cpp) equals the oracle's parse or raises its error, for
every flaw, position and parser piece size; and a source check that keeps every restart on reset_plan."""
import os
import re

import numpy as np
import pytest

from tests import test_gpu_late_fallback as late

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def parse_both(sc, oracle, path):
    from oracle.pyoracle import OracleError
    from screencounter_amd import _lib
    try:
        exp = ("ok",) + oracle.parse_fastq(path)
    except OracleError as e:
        exp = ("error", str(e))
    try:
        got = ("ok",) + sc.parse_fastq(path)
    except _lib.ScgError as e:
        assert e.code == _lib.SCG_ERR_IO, (e.code, str(e))
        got = ("error", str(e))
    return got, exp


def same(got, exp):
    if exp[0] == "error":
        return got == exp
    return got[0] == "ok" and np.array_equal(got[1], exp[1]) and np.array_equal(got[2], exp[2])


@pytest.mark.parametrize("piece_kb", [1, 7])
@pytest.mark.parametrize("scenario", late.SINGLE_SCENARIOS, ids=[s[0] for s in late.SINGLE_SCENARIOS])
def test_single_end_files_parse_like_the_oracle(sc, oracle, tmp_path, monkeypatch, scenario, piece_kb):
    monkeypatch.setenv("SCG_HOST_THREADS", str(late.HOST_THREADS))
    monkeypatch.setenv("SCG_FASTQ_PIECE_KB", str(piece_kb))
    path = late.write_single(str(tmp_path / "r.fastq"), scenario)
    got, exp = parse_both(sc, oracle, path)
    assert same(got, exp), (got[0], exp[0], got[1:] if got[0] == "error" else "", exp[1:] if exp[0] == "error" else "")
    kinds = set(scenario[1].values())
    assert (exp[0] == "error") == ("malformed" in kinds)
    if exp[0] == "ok":
        assert len(exp[2]) - 1 == late.N_READS


@pytest.mark.parametrize("piece_kb", [1, 7])
@pytest.mark.parametrize("scenario", late.PAIRED_SCENARIOS, ids=[s[0] for s in late.PAIRED_SCENARIOS])
def test_paired_files_parse_like_the_oracle(sc, oracle, tmp_path, monkeypatch, scenario, piece_kb):
    monkeypatch.setenv("SCG_HOST_THREADS", str(late.HOST_THREADS))
    monkeypatch.setenv("SCG_FASTQ_PIECE_KB", str(piece_kb))
    for path in late.write_paired(str(tmp_path), scenario):
        got, exp = parse_both(sc, oracle, path)
        assert same(got, exp), (path, got[0], exp[0])


def test_the_flaws_sit_behind_many_windows(tmp_path):
    """What makes those files late: with 3 host threads and pieces of 1 KB the parser's window is 3 KB (2 KB per mate of a
    paired run), and a flaw in the middle has more than 20 windows before it."""
    assert late.SINGLE_SCENARIOS[1][2] == 1 and late.PAIRED_SCENARIOS[1][3] == 1
    path = late.write_single(str(tmp_path / "r.fastq"), late.SINGLE_SCENARIOS[1])
    assert os.path.getsize(path) / 2 >= 20 * late.HOST_THREADS * 1024, os.path.getsize(path)
    for p in late.write_paired(str(tmp_path), late.PAIRED_SCENARIOS[1]):
        assert os.path.getsize(p) / 2 >= 20 * 2 * 1024, (p, os.path.getsize(p))


def test_restarts_clear_the_plan_through_reset_plan():
    """A restart that clears only the dense counters leaves the combinations of sparse mode (and batches still in flight)
    behind: every clear of a plan's counters in the host sources goes through reset_plan.  (scg_plan_reset, the ABI's own reset,
    is no restart: it clears on the caller's stream, in the caller's order, and is left out.)"""
    import glob
    csrc = os.path.join(ROOT, "screencounter_amd", "csrc")
    files = sorted(glob.glob(os.path.join(csrc, "*.cpp")) + glob.glob(os.path.join(csrc, "*.hpp")))
    assert len(files) >= 8, files
    text = "".join(open(f).read() for f in files)
    abi = re.search(r"^int scg_plan_reset\(.*?^\}\n", text, re.S | re.M)
    assert abi and abi.group(0).count("sparse_counts.clear()") == 1, "scg_plan_reset not found"
    text = text[:abi.start()] + text[abi.end():]
    m = re.search(r"^void reset_plan\(scg_plan\* P\) \{\n(.*?)^\}\n", text, re.S | re.M)
    assert m, "reset_plan not found"
    outside = text[:m.start()] + text[m.end():]
    assert "hipMemset(P->counters" in m.group(1)
    assert not re.search(r"hipMemset(Async)?\(\s*P->counters", outside), "counters cleared outside reset_plan"
    assert "sparse_counts.clear()" in m.group(1) and "sparse_counts.clear()" not in outside
