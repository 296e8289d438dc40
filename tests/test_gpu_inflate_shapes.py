"""The device's three DEFLATE decoders -- the per-wavefront one (SCG_INFLATE_LANES=0), the lane-parallel one (the default for
BGZF; in symbol mode stage 1 of the gzip path) and the two-stage gunzip kernels -- on streams zlib's deflate never writes
(tests/deflate_writer.py, tests/deflate_shapes.py; tests/test_deflate_shapes_cpu.py checks the same streams against zlib and
the host build first).  The device has no inflate-only entry point: the counting calls are the observer.  Every text is
ordinary 4-line FASTQ, every member's CRC-32 that of the intended text, so under SCG_DEVICE_INFLATE=2 / SCG_DEVICE_GUNZIP=2 a
passing call means that the device decoded every byte and that the sequence lines count like the oracle's.  All comparisons
are exact.  profiles/inflate_shapes_coverage.txt lists the shapes and each decoder's verdict."""
import numpy as np
import pytest

from tests import deflate_shapes as shapes

pytestmark = pytest.mark.gpu

TEMPLATE = shapes.TEMPLATE
DECODERS = {"lanes": None, "wavefront": "0"}            # SCG_INFLATE_LANES


@pytest.fixture(scope="module")
def pool():
    return shapes.make_pool()


@pytest.fixture(scope="module")
def bgzf_files(tmp_path_factory, oracle, pool):
    """{group: (path, expected counts, total, names of the crafted streams)}, written once."""
    d = tmp_path_factory.mktemp("bgzf_shapes")
    out = {}
    for k, (group, build) in enumerate(shapes.BGZF_GROUPS.items()):
        F = build(100 + k, pool)
        if F is None:
            continue
        path = str(d / ("%d.bgzf.gz" % k))
        open(path, "wb").write(F.finish())
        exp, total = oracle.count_single(F.reads, TEMPLATE, 2, pool, 1, True)
        assert total == len(F.reads) and exp.sum() > len(F.reads) // 3
        out[group] = (path, exp, total, [s[0] for s in F.streams])
    return out


@pytest.fixture(scope="module")
def gzip_text(pool):
    return shapes.GzipText(9, pool)


@pytest.fixture(scope="module")
def gzip_files(tmp_path_factory, oracle, pool, gzip_text):
    d = tmp_path_factory.mktemp("gzip_shapes")
    expected = {}                                            # (most cases hold the same reads: counted once)
    out = {}
    for k, (name, (data, raw, f, text, reads)) in enumerate(shapes.gzip_cases(gzip_text, pool).items()):
        path = str(d / ("%d.fastq.gz" % k))
        open(path, "wb").write(data)
        key = (len(reads), reads[0], reads[-1])
        if key not in expected:
            expected[key] = oracle.count_single(reads, TEMPLATE, 2, pool, 1, True)
            assert expected[key][1] == len(reads)
        out[name] = (path,) + tuple(expected[key])
    return out


def count(sc, path, pool):
    return sc.count_single_barcodes(path, TEMPLATE, 2, pool, 1, True, 4)


def rung_lines(capfd):
    return [line[len("[scg] rung "):] for line in capfd.readouterr().err.splitlines() if line.startswith("[scg] rung ")]


def outcome(sc, path, pool):
    try:
        c, t = count(sc, path, pool)
        return ("ok", t, c.tobytes())
    except sc.ScgError as e:
        return ("error", e.code, str(e))


@pytest.mark.parametrize("decoder", list(DECODERS))
@pytest.mark.parametrize("group", list(shapes.BGZF_GROUPS))
def test_bgzf_shapes_are_decoded_by_the_device(sc, gpu, pool, bgzf_files, monkeypatch, capfd, group, decoder):
    """Crafted members between zlib-written ones (records straddle them).  A decline of a valid stream is a bug: the strict
    switch turns it into an error here.  Whole file in one window, and in windows of 200 KB."""
    if group not in bgzf_files:
        pytest.skip("libdeflate.so.0 is not installed")
    path, exp, total, names = bgzf_files[group]
    monkeypatch.setenv("SCG_DEVICE_INFLATE", "2")
    if DECODERS[decoder] is not None:
        monkeypatch.setenv("SCG_INFLATE_LANES", DECODERS[decoder])
    monkeypatch.setenv("SCG_TRACE", "1")
    for window_kb in (None, 200):
        if window_kb:
            monkeypatch.setenv("SCG_WINDOW_KB", str(window_kb))
        capfd.readouterr()
        got, n = count(sc, path, pool)
        assert rung_lines(capfd) == ["device-inflate"], (group, decoder, window_kb)
        assert n == total, (group, decoder, window_kb)
        assert np.array_equal(got, exp), (group, decoder, window_kb)
    for name in names:
        print("bgzf | %s | %s | %s | taken" % (group, name, decoder))


# which gzip cases the device takes (its rungs under SCG_TRACE=1) and which it declines by design
TAKEN = ["device-gunzip"]
GZIP_VERDICTS = {
    "blocks of about 1 KB, chains through every chunk": TAKEN,
    "stored blocks across chunk boundaries": TAKEN,
    "long-code blocks": TAKEN,
    "one dynamic block": TAKEN,
    "fixed blocks only": TAKEN,
    "stored blocks only": TAKEN,
    "repeats across the boundary in the first headers": TAKEN,
    "a last chunk of 40 bits": TAKEN,
}


@pytest.mark.parametrize("case", list(GZIP_VERDICTS))
def test_gzip_shapes_on_the_device_path(sc, gpu, pool, gzip_files, monkeypatch, capfd, case):
    """About 0.9 MB of text in chunks of 4 KB.  With the default switch the counts are the oracle's whoever decodes; with
    SCG_DEVICE_GUNZIP=2 the call gives those counts or the hand-back error, never other counts; and who decoded is pinned."""
    path, exp, total = gzip_files[case]
    monkeypatch.setenv("SCG_PGZIP_CHUNK_KB", "64")
    monkeypatch.setenv("SCG_DGZIP_CHUNK_KB", "4")
    monkeypatch.setenv("SCG_TRACE", "1")
    capfd.readouterr()
    got, n = count(sc, path, pool)
    rungs = rung_lines(capfd)
    print("gzip | %s | %s" % (case, rungs))
    assert n == total and np.array_equal(got, exp), case
    assert rungs == GZIP_VERDICTS[case], (case, rungs)
    monkeypatch.setenv("SCG_DEVICE_GUNZIP", "2")
    taken = GZIP_VERDICTS[case] == TAKEN
    settings = [(None, None)]
    if case.startswith("blocks of about 1 KB"):
        settings += [("1", None), ("3", "200")]               # the tails' scan over groups of 1 and of 3 chunks; 200 KB windows
    for tail_group, window_kb in settings:
        if tail_group:
            monkeypatch.setenv("SCG_DGZIP_TAIL_GROUP", tail_group)
        if window_kb:
            monkeypatch.setenv("SCG_WINDOW_KB", window_kb)
        if taken:
            got, n = count(sc, path, pool)
            assert n == total and np.array_equal(got, exp), (case, tail_group, window_kb)
        else:
            with pytest.raises(sc.ScgError) as e:
                count(sc, path, pool)
            assert "SCG_DEVICE_GUNZIP=2" in str(e.value)


@pytest.mark.parametrize("decoder", list(DECODERS))
@pytest.mark.parametrize("kind", ["distance beyond the start", "symbol 286"])
def test_invalid_bgzf_members_end_like_the_sequential_reader(sc, gpu, pool, tmp_path, monkeypatch, capfd, kind, decoder):
    """A distance one byte beyond the member's start; a fixed block that uses literal/length symbol 286: the device hands the
    file back, and the call ends exactly as the sequential reader's (SCG_DEVICE_SCAN=0) -- error code and message."""
    F = shapes.bgzf_invalid(kind, 5, pool)
    path = str(tmp_path / "invalid.bgzf.gz")
    open(path, "wb").write(F.finish())
    monkeypatch.setenv("SCG_DEVICE_SCAN", "0")
    want = outcome(sc, path, pool)
    monkeypatch.delenv("SCG_DEVICE_SCAN")
    assert want[0] == "error"
    if DECODERS[decoder] is not None:
        monkeypatch.setenv("SCG_INFLATE_LANES", DECODERS[decoder])
    monkeypatch.setenv("SCG_TRACE", "1")
    capfd.readouterr()
    got = outcome(sc, path, pool)
    rungs = rung_lines(capfd)
    print("bgzf | invalid | %s | %s | %s, %r" % (kind, decoder, rungs[:2], want[2]))
    assert got == want
    assert rungs[:2] == ["device-inflate", "device-inflate: declined -> host-threads"]


def test_a_second_gzip_member_may_not_reach_into_the_first(sc, gpu, pool, gzip_text, tmp_path, monkeypatch, capfd):
    """Two members; the second, in its fourth chunk or later, copies from one byte in front of itself.  The first member's text
    lies right there in the device's buffer, and the trailer carries the CRC-32 of what reading it would give: the `avail`
    rule of the tails is all that tells -- and zlib calls the file an error."""
    data, raw2, f = shapes.gzip_two_members_reaching_back(gzip_text, 3, pool)
    path = str(tmp_path / "two.fastq.gz")
    open(path, "wb").write(data)
    monkeypatch.setenv("SCG_PGZIP_CHUNK_KB", "64")
    monkeypatch.setenv("SCG_DGZIP_CHUNK_KB", "4")
    monkeypatch.setenv("SCG_DEVICE_SCAN", "0")
    want = outcome(sc, path, pool)
    monkeypatch.delenv("SCG_DEVICE_SCAN")
    assert want[0] == "error"
    monkeypatch.setenv("SCG_TRACE", "1")
    for tail_group in (None, "1", "3"):
        if tail_group:
            monkeypatch.setenv("SCG_DGZIP_TAIL_GROUP", tail_group)
        capfd.readouterr()
        got = outcome(sc, path, pool)
        rungs = rung_lines(capfd)
        print("gzip | invalid | second member reaches into the first | %s, %r" % (rungs[:2], want[2]))
        assert got == want
        # (the first member is the device's; the second is refused once its tails are made)
        assert rungs[:2] == ["device-gunzip", "device-gunzip: declined -> host-threads"]
