"""The gzip container parsers every reader shares (csrc/scg_gzip.h: member header, BGZF size subfield, trailer) on
headers built by hand in buffers of exactly the announced size: each optional field alone and all together, XLEN 0 and
65535, the BC subfield in every position and cut short, a buffer that ends at every byte of a header, unterminated
names, reserved flags.  Host code only (tests/gzip_container_harness.cpp): run natively and under AddressSanitizer +
UBSan, which see any byte read beyond a buffer."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("build", ["native", "asan"])
def test_container_parsers(build, tmp_path):
    gxx = shutil.which("g++")
    if not gxx:
        pytest.skip("no g++")
    exe = str(tmp_path / f"gzip_container_{build}")
    flags = ["-O2"] if build == "native" else ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer"]
    subprocess.run([gxx, "-std=c++17", *flags, "-o", exe, os.path.join(ROOT, "tests", "gzip_container_harness.cpp"), "-ldl"],
                   check=True, capture_output=True, text=True)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-2000:])
    assert r.stdout.startswith("ok:")
