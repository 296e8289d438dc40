"""Hand-written DEFLATE streams (tests/deflate_writer.py, tests/deflate_shapes.py) before they go anywhere near a device:
zlib must read every valid one as exactly the intended text and refuse every invalid one; the shapes the streams are
there for must really occur in them (the writer's own record of what it emitted, checked as conditions); and the host
build of the per-wavefront decoder (csrc/scg_inflate.h, lane widths 1, 7 and 64) must give zlib's verdict and the intended
text for each, under AddressSanitizer and UBSan.  Streams over arbitrary byte alphabets are here too.  No device needed."""
import os
import random
import shutil
import struct
import subprocess
import zlib

import pytest

from tests import deflate_shapes as shapes
from tests.deflate_writer import (Block, Features, Script, bounded_lengths, check_lengths, deflate, expand, inverted_lengths,
                                  limited_lengths, tokenize, zlib_says)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def arbitrary_streams():
    """Streams that are no FASTQ: every byte value, runs, random data, through every knob of the matcher and the writer."""
    rng = random.Random(77)
    out = []
    texts = {
        "every byte": bytes(range(256)) * 12,
        "random": bytes(rng.randrange(256) for _ in range(8000)),
        "geometric": bytes(min(255, int(rng.expovariate(0.05))) for _ in range(20000)),
        "runs": b"".join(bytes([rng.randrange(256)]) * rng.randrange(1, 600) for _ in range(60)),
        "short periods": b"".join((bytes(rng.randrange(256) for _ in range(rng.randrange(1, 70))) * 40)[:rng.randrange(3, 900)] for _ in range(50)),
        "empty": b"",
        "one byte": b"\xff",
    }
    knobs = [dict(), dict(farthest=True), dict(overlap=True), dict(min_len=4, max_len=17), dict(max_dist=300), dict(min_len=200)]
    for name, text in texts.items():
        for k, knob in enumerate(knobs):
            tokens = tokenize(text, **knob)
            assert expand(tokens) == text
            sizes = [rng.randrange(1, 400) for _ in range(50)]
            kinds = [rng.choice(["stored", "fixed", "dynamic"]) for _ in range(31)]
            blocks = []
            at = 0
            for j in range(10 ** 6):
                if at >= len(tokens) and j:
                    break
                part = tokens[at:at + sizes[j % 50]]
                at += sizes[j % 50]
                kind = kinds[j % 31]
                if kind == "stored":
                    if any(t.__class__ is not int for t in part):
                        kind = "dynamic"
                    else:
                        blocks.append(Block("stored", part))
                        continue
                blocks.append(Block(kind, part, header=("zlib", "plain", "cross")[(j + k) % 3], len258=("285", "284+31")[j % 2],
                                    max_bits=(15, 9, 12)[k % 3], hlit=286 if j % 5 == 0 else None, hdist=30 if j % 7 == 0 else None))
            blocks[-1].final = True
            raw, f = deflate(blocks)
            out.append(("%s / %d" % (name, k), raw, text, f))
    # long codes over a byte alphabet: the frequent bytes on the 15-bit codes
    text = texts["geometric"]
    tokens = tokenize(text, farthest=True)
    ll, dl = shapes.long_code_lengths(tokens)
    raw, f = deflate([Block("dynamic", tokens, lit_lens=ll, dist_lens=dl, final=True)])
    out.append(("geometric / long codes", raw, text, f))
    # invalid ones: what zlib names "over-subscribed", "incomplete", "missing end-of-block", "too far back", a bad stored length
    lf = [0] * 286
    for b in b"abcabcabc":
        lf[b] += 1
    lf[256] = 1
    good = limited_lengths(lf)
    over = list(good); over[ord("a")] = 1; over[ord("b")] = 1; over[ord("c")] = 2
    thin = list(good); thin[ord("a")] += 1
    for name, lens in (("over-subscribed", over), ("incomplete", thin)):
        raw, f = deflate([Block("dynamic", list(b"abcabcabc"), lit_lens=lens, dist_lens=[0], check=False, final=True)])
        out.append(("invalid: " + name, raw, None, f))
    s = Script(check=False)
    s.lit(b"abc").copy(5, 4)
    raw, f = deflate([Block("fixed", s.tokens, final=True)])
    out.append(("invalid: too far back", raw, None, f))
    raw, f = deflate([Block("stored", b"hello", final=True)])
    raw = bytearray(raw); raw[3] ^= 1
    out.append(("invalid: stored lengths", bytes(raw), None, f))
    raw, f = deflate([Block("fixed", list(b"ab") + [("code", 287)] + list(b"c"), final=True)])
    out.append(("invalid: symbol 287", raw, None, f))
    return out


@pytest.fixture(scope="module")
def streams():
    """Every stream of both tiers, built once: (name, container, raw stream, intended text or None, Features)."""
    pool = shapes.make_pool()
    out = []
    for k, (group, build) in enumerate(shapes.BGZF_GROUPS.items()):
        F = build(100 + k, pool)
        if F is None:
            continue
        whole = F.finish()
        assert zlib.decompress(whole, 31) is not None
        out += [("bgzf", group + ": " + n, raw, text, f) for n, raw, text, f in F.streams]
    for kind in ("distance beyond the start", "symbol 286"):
        F = shapes.bgzf_invalid(kind, 5, pool)
        out += [("bgzf", "invalid: " + n, raw, text, f) for n, raw, text, f in F.streams]
    G = shapes.GzipText(9, pool)
    for name, (data, raw, f, text, reads) in shapes.gzip_cases(G, pool).items():
        out.append(("gzip", name, raw, text, f))
    data, raw2, f = shapes.gzip_two_members_reaching_back(G, 3, pool)
    out.append(("gzip", "invalid: second member reaches into the first", raw2, None, f))
    out += [("other", n, raw, text, f) for n, raw, text, f in arbitrary_streams()]
    return out


def test_zlib_reads_every_valid_stream_and_refuses_every_invalid_one(streams):
    n_valid = n_invalid = 0
    for container, name, raw, text, f in streams:
        d = zlib.decompressobj(-15)
        if text is None:
            with pytest.raises(zlib.error):
                d.decompress(raw)
            n_invalid += 1
        else:
            assert d.decompress(raw) == text, name
            assert d.eof and not d.unused_data, name
            n_valid += 1
    print(n_valid, "valid,", n_invalid, "invalid")
    assert n_valid >= 60 and n_invalid >= 8


@pytest.mark.parametrize("container", ["bgzf", "gzip"])
def test_the_shapes_really_occur(streams, container):
    """Conditions on what the writer emitted in the VALID streams of a container, not a report."""
    f = Features()
    mine = [s for s in streams if s[0] == container and s[3] is not None]
    for s in mine:
        f.merge(s[4])
    assert f.max_lit_code == 15 and f.max_dist_code == 15
    assert f.long_pair_blocks >= 1                       # a literal/length code > 10 bits and a distance code > 8 bits used in one block
    assert {1, 32768, 32767} <= f.distances
    assert 3 in f.lengths
    assert set(range(8)) <= f.eob_before_stored          # a stored block behind a block that ends at each bit offset
    assert f.blocks["stored"] and f.blocks["fixed"] and f.blocks["dynamic"]
    assert 258 in f.lengths and f.spell258 == {"285", "284+31"}
    assert f.crossing_repeats == {16, 17, 18}
    if container == "gzip":
        return
    assert f.length_symbols == set(range(257, 286))
    assert {2, 24577} <= f.distances and f.reach_start >= 1
    assert f.longest_18 == 138
    assert {286} <= f.hlit and {30, 1} <= f.hdist and {8, 19} <= f.hclen
    assert f.no_distance_code >= 1 and f.one_bit_distance_code >= 1 and f.eob_only_dynamic >= 1
    assert f.long_length_only_blocks >= 1
    assert f.empty_blocks["stored"] and f.empty_blocks["fixed"] and f.empty_blocks["dynamic"]
    assert f.full_width_over_512 >= 1                    # 15 + 5 + 15 + 13 bits across a multiple of 512 bytes of the payload
    short258 = by_name_of(mine)["extremes: length 258 as 284 + 31 on short codes"][4]
    assert short258.spell258 == {"284+31"} and short258.max_lit_code <= 10          # (within the lane decoder's primary table)
    assert f.header_styles == {"plain", "zlib", "cross"}
    by_name = {s[1]: s for s in mine}
    for extra in (0, 1, 7, 8):
        assert len(by_name["ring and payload edges: payload of 512 k + %d bytes" % extra][2]) % 512 == extra
    assert by_name["ring and payload edges: end-of-block on the last bit of the payload's last byte"][4].eob_offsets[-1] == 0
    assert by_name["ring and payload edges: end-of-block on the first bit of the payload's last byte"][4].eob_offsets[-1] == 1
    # dist < len for each of these distances; >= 200 matches in a row, each reading what the one before it wrote -- through
    # Huffman codes of ordinary size and through two-bit matches (64 to a batch of the lane decoder: its slots fill up)
    chains = by_name["overlap and chains: overlap and chains"][4]
    assert {1, 2, 3, 4, 5, 6, 7, 8, 9, 63, 64, 65} <= chains.overlap_distances
    assert chains.longest_match_chain >= 400
    assert by_name["overlap and chains: chains in one-bit codes"][4].longest_match_chain >= 500


def by_name_of(streams):
    return {s[1]: s for s in streams}


def test_gzip_shapes_sit_where_the_chunks_need_them(streams):
    by_name = {s[1]: s for s in streams if s[0] == "gzip"}
    name, raw, f = "blocks of about 1 KB, chains through every chunk", None, None
    _, _, raw, _, f = by_name[name]
    assert len(raw) > 32 * 4096
    starts = [b // 8 // 4096 for b in f.block_starts]
    assert max(starts.count(c) for c in set(starts)) >= 3                     # several block starts in a chunk
    assert f.block_starts[-1] // 8 // 4096 == (len(raw) - 1) // 4096          # the final dynamic block begins inside the last chunk
    assert len(by_name["a last chunk of 40 bits"][2]) % 4096 == 5
    assert by_name["one dynamic block"][4].blocks == {"stored": 0, "fixed": 0, "dynamic": 1}
    assert by_name["fixed blocks only"][4].blocks["dynamic"] == 0 and by_name["stored blocks only"][4].blocks["dynamic"] == 0


def test_the_writer_refuses_what_it_is_not_told_to_allow():
    with pytest.raises(ValueError):
        check_lengths([1, 1, 1])
    with pytest.raises(ValueError):
        check_lengths([2, 2, 2])
    check_lengths([1])
    check_lengths([0, 0])
    check_lengths(inverted_lengths(list(range(286)), 286))
    check_lengths(bounded_lengths([1] * 100, 6, 9))
    assert max(limited_lengths([2 ** k for k in range(40)], 15)) == 15
    check_lengths(limited_lengths([2 ** k for k in range(40)], 15))
    with pytest.raises(ValueError):
        Script().lit(b"ab").copy(3, 3)


@pytest.fixture(scope="module")
def harness(tmp_path_factory):
    gxx = shutil.which("g++")
    if not gxx:
        pytest.skip("no g++")
    exe = str(tmp_path_factory.mktemp("inflate_shapes") / "inflate_harness")
    cmd = [gxx, "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
           os.path.join(ROOT, "tests", "inflate_harness.cpp"), "-lz", "-o", exe]
    subprocess.run(cmd, check=True, capture_output=True, text=True)
    return exe


def test_wavefront_decoder_on_the_host_gives_zlibs_verdict(streams, harness, tmp_path):
    path = str(tmp_path / "streams.bin")
    with open(path, "wb") as out:
        for container, name, raw, text, f in streams:
            # (an invalid stream announces the size its tokens stand for, so that the decoder gets as far as the defect)
            intended = text if text is not None else b"?" * f.n_bytes
            out.write(struct.pack("<IIB", len(raw), len(intended), text is not None) + raw + intended)
    r = subprocess.run([harness, "--streams", path], capture_output=True, text=True, timeout=600)
    detail = r.stderr[-2000:]
    if "entry" in detail:
        k = int(detail.split("entry ")[1].split(":")[0].split()[0])
        detail += " (" + streams[k][1] + ")"
    assert r.returncode == 0, detail
    assert r.stdout.startswith("ok: %d streams" % len(streams))
