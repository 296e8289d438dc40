"""The SCG_* switches (csrc/scg_env.h): every switch's parsing rule, the snapshot rules of EnvScope / env(), and where
the switches may be read and are documented.  Host code only (tests/env_harness.cpp): run natively and under
AddressSanitizer + UBSan.

RULES below was written from the parsing code the switches had before scg_env.h existed, each where it was used; the
file:line next to a switch names that rule in commit c34134e.  A value is what the harness prints for the switch; a
dict gives its second facet too (NAME.set, NAME.strict)."""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "screencounter_amd", "csrc")
UNSET = None
BIG = "1000000"


FIRST_NOT_0 = {UNSET: 1, "": 1, "0": 0, "1": 1, "2": 1, "01": 0, BIG: 1, "abc": 1}      # e && *e == '0' alone has an effect; empty counts as on
FLAG = {UNSET: 0, "": 0, "0": 0, "1": 1, "2": 1, "01": 0, BIG: 1, "abc": 1}             # e && *e && *e != '0'


def _two_facets(name, facet):    # on unless the first character is '0'; strict when it is '2'
    f = name + facet
    return {UNSET: {name: 1, f: 0}, "": {name: 1, f: 0}, "0": {name: 0, f: 0}, "1": {name: 1, f: 0}, "2": {name: 1, f: 1}, "20": {name: 1, f: 1},
            "02": {name: 0, f: 0}, BIG: {name: 1, f: 0}, "abc": {name: 1, f: 0}}


def _set(v, s):
    return {"SCG_DEVICE": v, "SCG_DEVICE.set": s}


def _chunk(v, s):
    return {"SCG_DGZIP_CHUNK_KB": v, "SCG_DGZIP_CHUNK_KB.set": s}


def _list(v, s):
    return {"SCG_DEVICES": "[" + v + "]", "SCG_DEVICES.set": s}


RULES = {
    # scg_internal.hpp:97-99 (env && *env -> atoi); scg_results.cpp:77 (set and non-empty, SCG_DEVICES unset or empty -> that device alone)
    "SCG_DEVICE": {UNSET: _set(-1, 0), "": _set(-1, 0), "0": _set(0, 1), "1": _set(1, 1), "2": _set(2, 1), "-1": _set(-1, 1), BIG: _set(1000000, 1),
                   "abc": _set(0, 1)},
    # scg_results.cpp:60-62 (env && *env; the list itself is parsed, and its errors worded, by device_list)
    "SCG_DEVICES": {UNSET: _list("", 0), "": _list("", 0), "0": _list("0", 1), "1": _list("1", 1), "2": _list("2", 1), "all": _list("all", 1),
                    "0,0,1": _list("0,0,1", 1), BIG: _list(BIG, 1), "abc": _list("abc", 1)},
    # scg_fastq.cpp:224-228 (env && *env, atoi >= 1; else sized from the machine)
    "SCG_HOST_THREADS": {UNSET: 0, "": 0, "0": 0, "1": 1, "2": 2, "-3": 0, BIG: 1000000, "abc": 0},
    # scg_internal.hpp:338-339 (plain atoi whenever set: empty gives 0, not 20)
    "SCG_REPLICA_ADDR_LOG2": {UNSET: 20, "": 0, "0": 0, "1": 1, "2": 2, "-5": -5, BIG: 1000000, "abc": 0},
    # scg_plan.cpp:20-22 (e && *e, atoll clamped to [0, 2^30]; else 2^26)
    "SCG_DENSE_CELLS": {UNSET: 1 << 26, "": 1 << 26, "0": 0, "1": 1, "2": 2, "-1": 0, str(1 << 30): 1 << 30, str((1 << 30) + 1): 1 << 30,
                        "99999999999": 1 << 30, BIG: 1000000, "abc": 0},
    # scg_plan.cpp:405 (unset or empty: the size rule; else on unless the first character is '0')
    "SCG_TALLY": {UNSET: -1, "": -1, "0": 0, "1": 1, "2": 1, "01": 0, BIG: 1, "abc": 1},
    # scg_kernels.hip:1118 ((size_t)atoi whenever set: a negative value wraps)
    "SCG_EXTRA_LDS_KB": {UNSET: 0, "": 0, "0": 0, "1": 1, "2": 2, "16": 16, "-1": 2 ** 64 - 1, BIG: 1000000, "abc": 0},
    # scg_kernels.hip:1239 (e && *e -> atoi; else -1)
    "SCG_DUAL_TWO_TILES": {UNSET: -1, "": -1, "0": 0, "1": 1, "2": 2, "-1": -1, BIG: 1000000, "abc": 0},
    # scg_inflate.hip:812-813
    "SCG_INFLATE_LANES": FIRST_NOT_0,
    # scg_library.cpp:22 (atoi >= 2; else the tiers by library size, printed as 0)
    "SCG_TABLE_FACTOR": {UNSET: 0, "": 0, "0": 0, "1": 0, "2": 2, "3": 3, "-2": 0, BIG: 1000000, "abc": 0},
    # scg_library.cpp:513-514 (atoi in [4, SCG_SEED_LEN = 10]; else SCG_SEED_LEN - 1)
    "SCG_SEED_MAX": {UNSET: 9, "": 9, "0": 9, "1": 9, "2": 9, "3": 9, "4": 4, "10": 10, "11": 9, BIG: 9, "abc": 9},
    # scg_ingest.cpp:553-554 (atof clamped to >= 0 whenever set; 0 = never; else 8)
    "SCG_GZIP_WHOLE_GB": {UNSET: 8.0, "": 0.0, "0": 0.0, "1": 1.0, "2": 2.0, "0.5": 0.5, "-1": 0.0, BIG: 1e6, "abc": 0.0},
    # scg_gzip.h:92-93
    "SCG_LIBDEFLATE": FIRST_NOT_0,
    # scg_internal.hpp:78-79
    "SCG_TRACE": FLAG,
    # scg_kernels.hip:1131-1132
    "SCG_FORCE_GENERAL": FLAG,
    # scg_internal.hpp:511-512 (first character != '0': an empty value is on)
    "SCG_DEVICE_SCAN": FIRST_NOT_0,
    # scg_internal.hpp:513
    "SCG_HOST_SCAN": FIRST_NOT_0,
    # scg_internal.hpp:514; scg_dgzip.cpp:95-96 (e && *e == '0'): the same rule twice
    "SCG_BUFFER_CACHE": FIRST_NOT_0,
    # scg_internal.hpp:515-516
    "SCG_DEVICE_INFLATE": _two_facets("SCG_DEVICE_INFLATE", ".strict"),
    # scg_dgzip.cpp:431-432 (off for '0' alone); scg_internal.hpp:517 (strict for '2')
    "SCG_DEVICE_GUNZIP": _two_facets("SCG_DEVICE_GUNZIP", ".strict"),
    # scg_ingest.cpp:593-594
    "SCG_PGZIP": FIRST_NOT_0,
    # scg_internal.hpp:518 (atol clamped to >= 0 whenever set; 0 = the built-in sizes)
    "SCG_WINDOW_KB": {UNSET: 0, "": 0, "0": 0, "1": 1, "2": 2, "-4": 0, BIG: 1000000, "abc": 0},
    # scg_fastq.cpp:294-298 (atol > 0; else 32 MB)
    "SCG_FASTQ_PIECE_KB": {UNSET: 32768, "": 32768, "0": 32768, "-1": 32768, "1": 1, "2": 2, BIG: 1000000, "abc": 32768},
    # scg_plan.cpp:466-468 (e && *e, atoi clamped to [0, 61]; else 61)
    "SCG_TEST_RANDOM_TAG_BITS": {UNSET: 61, "": 61, "0": 0, "1": 1, "2": 2, "-1": 0, "61": 61, "62": 61, BIG: 61, "abc": 0},
    # scg_dgzip.cpp:168-171 (set at all, whatever the value: files from 64 bytes; the value applies from 4 on; else 64)
    "SCG_DGZIP_CHUNK_KB": {UNSET: _chunk(64, 0), "": _chunk(64, 1), "0": _chunk(64, 1), "1": _chunk(64, 1), "2": _chunk(64, 1), "3": _chunk(64, 1),
                           "4": _chunk(4, 1), BIG: _chunk(1000000, 1), "abc": _chunk(64, 1)},
    # scg_dgzip.cpp:172 (atol clamped to >= 1 whenever set; else 32)
    "SCG_DGZIP_TAIL_GROUP": {UNSET: 32, "": 1, "0": 1, "1": 1, "2": 2, "-7": 1, BIG: 1000000, "abc": 1},
    # scg_dgzip.cpp:173 (atol clamped to >= 0 whenever set; else 32)
    "SCG_DGZIP_MIN_MEMBER_CHUNKS": {UNSET: 32, "": 0, "0": 0, "1": 1, "2": 2, "-1": 0, BIG: 1000000, "abc": 0},
    # scg_dgzip.cpp:178-179 (atol >= 4; else 512 MB)
    "SCG_DGZIP_GROUP_KB": {UNSET: 524288, "": 524288, "0": 524288, "1": 524288, "2": 524288, "3": 524288, "4": 4, BIG: 1000000, "abc": 524288},
    # scg_pgzip.cpp:123-126 (atol >= 1; else by file size and threads, printed as 0)
    "SCG_PGZIP_CHUNK_KB": {UNSET: 0, "": 0, "0": 0, "-1": 0, "1": 1, "2": 2, BIG: 1000000, "abc": 0},
    # scg_pgzip.cpp:165 (atol >= 1; else by chunk size, printed as 0)
    "SCG_PGZIP_CAP_KB": {UNSET: 0, "": 0, "0": 0, "-1": 0, "1": 1, "2": 2, BIG: 1000000, "abc": 0},
}
# (SCG_ABLATE, scg_plan.cpp:31-34, exists in -DSCG_ABLATE measurement builds only: plain atoi whenever set)


def _build(tmp_path_factory, build):
    gxx = shutil.which("g++")
    if not gxx:
        pytest.skip("no g++")
    exe = str(tmp_path_factory.mktemp("env") / f"env_harness_{build}")
    flags = ["-O2"] if build == "native" else ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer"]
    subprocess.run([gxx, "-std=c++17", "-Wall", "-Wextra", *flags, "-o", exe, os.path.join(ROOT, "tests", "env_harness.cpp"), "-lpthread"],
                   check=True, capture_output=True, text=True)
    return exe


@pytest.fixture(scope="module")
def native(tmp_path_factory):
    return _build(tmp_path_factory, "native")


@pytest.fixture(scope="module")
def asan(tmp_path_factory):
    return _build(tmp_path_factory, "asan")


def _run(exe, mode, **switches):
    env = {k: v for k, v in os.environ.items() if not k.startswith("SCG_")}
    env.update({k: v for k, v in switches.items() if v is not UNSET})
    r = subprocess.run([exe, mode], capture_output=True, text=True, timeout=60, env=env)
    assert r.returncode == 0, (switches, r.stdout[-2000:], r.stderr[-2000:])
    return r.stdout


def _read(exe, **switches):
    return dict(pair.split("=", 1) for pair in _run(exe, "read", **switches).split())


def _same(printed, expected):
    return float(printed) == expected if isinstance(expected, float) else printed == str(expected)


def _expected(name, value):
    exp = RULES[name][value]
    return exp if isinstance(exp, dict) else {name: exp}


def test_every_switch_has_rules():
    """RULES covers the switches of scg_env.h, each with unset, empty, 0, 1, 2, a large value and text."""
    assert set(RULES) == _header_names() - {"SCG_ABLATE"}
    for name, rows in RULES.items():
        assert {UNSET, "", "0", "1", "2", BIG, "abc"} <= set(rows), name


@pytest.mark.parametrize("name", sorted(RULES))
def test_parse_rules(native, name):
    defaults = _read(native)
    for key, exp in _expected(name, UNSET).items():
        assert _same(defaults[key], exp), (name, "unset", key, defaults[key], exp)
    for value in RULES[name]:
        got = _read(native, **{name: value})
        want = _expected(name, value)
        for key in got:            # the switch reads as the old rule says, and no other switch moves
            if key in want:
                assert _same(got[key], want[key]), (name, value, key, got[key], want[key])
            else:
                assert got[key] == defaults[key], (name, value, key, got[key], defaults[key])


@pytest.mark.parametrize("build", ["native", "asan"])
def test_scope_rules(build, request):
    exe = request.getfixturevalue(build)
    assert _run(exe, "scopes", SCG_SEED_MAX="4").startswith("ok:")
    assert _run(exe, "first", SCG_SEED_MAX="4").startswith("ok:")


def test_read_under_sanitizers(native, asan):
    """Every switch at once -- empty, text, out of range, large -- reads the same with and without the sanitizers."""
    for value in ("", "abc", "-1", "2", BIG):
        everything = {name: value for name in RULES}
        assert _read(asan, **everything) == _read(native, **everything), value
    assert _read(asan) == _read(native)


# ---- where the switches are read, and where they are documented ----

def _sources():
    for f in sorted(os.listdir(CSRC)):
        if f.endswith((".h", ".hpp", ".cpp", ".hip")):
            yield f, open(os.path.join(CSRC, f)).read()


def _header_names():
    return set(re.findall(r'"(SCG_[A-Z0-9_]+)"', open(os.path.join(CSRC, "scg_env.h")).read()))


def test_getenv_only_in_scg_env_h():
    assert [f for f, text in _sources() if "getenv" in text] == ["scg_env.h"]


def test_no_second_mechanism():
    assert [f for f, text in _sources() if re.search(r"\bSwitches\b", text)] == []


def test_design_table_lists_every_switch():
    """The table of DESIGN.md §5.1 has one row per switch of scg_env.h, and the names read outside the library (SCG_LIB,
    -DSCG_STAGE_BLOCK) are not in it."""
    design = open(os.path.join(ROOT, "DESIGN.md")).read()
    rows = re.findall(r"^\| `(SCG_[A-Z0-9_]+)` \| (setting|tuning aid|test hook) \|", design, re.M)
    names = [n for n, _ in rows]
    assert len(names) == len(set(names))
    assert set(names) == _header_names()
    assert "SCG_LIB" not in names and "SCG_STAGE_BLOCK" not in names
    # the class in the table is the class in the header's comment
    header = open(os.path.join(CSRC, "scg_env.h")).read()
    for name, cls in rows:
        line = next(ln for ln in header.splitlines() if re.search(r"// %s\b" % name, ln))
        assert "(" + cls in line, (name, cls, line)
