"""The hand-written DEFLATE streams of tests/test_deflate_shapes_cpu.py and tests/test_gpu_inflate_shapes.py: shapes that
zlib's deflate never writes (deflate_writer.py writes them), as BGZF members inside ordinary 4-line FASTQ files and as
ordinary gzip files.  Every builder returns the file's bytes, the reads in it (for the oracle), and per crafted stream its
name, raw bytes, intended text (None = meant to be invalid) and Features."""
import ctypes
import random
import zlib

from tests import gen
from tests.deflate_writer import (Block, Features, Script, bgzf_member, bounded_lengths, deflate, gzip_member, inverted_lengths,
                                  limited_lengths, zlib_says, LEN_BASE, LEN_SYM, DIST_SYM)

TEMPLATE = "ACGTACGA" + "-" * 12 + "TGCATGCA"


def make_pool(seed=5):
    return gen.make_pool(random.Random(seed), 60, 12, "ACGT")


def fixed_read(rng, pool, length):
    """A read of exactly `length` bases: the filled template somewhere in random bases, on either strand, now and then mutated."""
    core = TEMPLATE.replace("-" * 12, rng.choice(pool))
    if rng.random() < 0.2:
        j = rng.randrange(len(core))
        core = core[:j] + rng.choice("ACGTN") + core[j + 1:]
    left = rng.randrange(length - len(core) + 1)
    r = gen.rand_seq(rng, left) + core + gen.rand_seq(rng, length - len(core) - left)
    return gen.rc(r) if rng.random() < 0.5 else r


def reads_of(rng, pool, n):
    return gen.make_reads(rng, TEMPLATE, [pool], n, 2, 0.03, 0.01, 0.02, 0.1, 40)


def name_of(rng, style, i=0):
    if style == "plain":
        return b"r%d some comment" % i
    if style == "long":
        return bytes(rng.choice(b"abcdefghijklmnopqrstuvwxyzABCDEFGHIJKLMNOPQRSTUVWXYZ0123456789:_/ ") for _ in range(rng.randrange(150, 240)))
    if style == "low":                                    # nothing above 't' (116)
        return bytes(rng.randrange(32, 117) for _ in range(rng.randrange(10, 40)))
    return bytes(rng.choice(ANY_BYTE) for _ in range(rng.randrange(10, 80)))      # any byte but \n


ANY_BYTE = bytes(b for b in range(256) if b != 10)


def qual_of(rng, n, style):
    if style == "geometric":
        return bytes(33 + min(93, int(rng.expovariate(0.12))) for _ in range(n))
    if style == "low":
        return bytes(33 + min(84, int(rng.expovariate(0.2))) for _ in range(n))
    return bytes(rng.choice(b"IIIIIIIIFFFF:,#") if rng.random() < 0.8 else rng.randrange(33, 127) for _ in range(n))     # skewed


def record(name, read, qual):
    return b"@" + name + b"\n" + read.encode() + b"\n+\n" + qual + b"\n"


class BgzfFile:
    """A BGZF file put together from zlib-written members and crafted ones over one continuous text.  A zlib member may
    hold back its last bytes for the member behind it, so that records straddle members (and the windows' carries happen)."""

    def __init__(self, rng, pool):
        self.rng, self.pool = rng, pool
        self.parts, self.reads, self.streams = [], [], []
        self.pending = b""
        self.serial = 0

    def records(self, n, names="any", quals="geometric", reads=None):
        reads = reads if reads is not None else reads_of(self.rng, self.pool, n)
        out = b""
        for r in reads:
            r = r or "A"
            self.reads.append(r)
            out += record(name_of(self.rng, names, self.serial), r, qual_of(self.rng, len(r), quals))
            self.serial += 1
        return out

    def zlib(self, n=12, hold=None, level=6, **kw):
        data = self.pending + self.records(n, **kw)
        hold = self.rng.randrange(1, 40) if hold is None else hold
        keep = len(data) - hold
        co = zlib.compressobj(level, zlib.DEFLATED, -15)
        self.parts.append(bgzf_member(co.compress(data[:keep]) + co.flush(), data[:keep]))
        self.pending = data[keep:]

    def crafted(self, name, blocks, text, valid=True, crc_text=None, size=None):
        """A member of `blocks`; text: what they are meant to give (it includes self.pending if the script began with it);
        crc_text: the text whose CRC-32 the trailer carries, if not that one; size: the bytes an invalid stream would give a
        decoder that overlooked its defect, if not those its tokens stand for (Features.n_bytes)."""
        blocks[-1].final = True
        raw, f = deflate(blocks)
        if size is not None:
            f.n_bytes = size
        if valid:
            assert zlib_says(raw) == bytes(text), name
        else:
            assert zlib_says(raw) is None, name
        self.streams.append((name, raw, bytes(text) if valid else None, f))
        self.parts.append(bgzf_member(raw, bytes(text) if crc_text is None else crc_text))
        self.pending = b""

    def script(self, check=True):
        s = Script(check)
        s.lit(self.pending)
        return s

    def rec(self, s, read, name=None, qual=None, **knobs):
        """An ordinary record appended to script s through the matcher."""
        self.reads.append(read)
        s.auto(record(name if name is not None else name_of(self.rng, "any"), read, qual if qual is not None else qual_of(self.rng, len(read), "geometric")), **knobs)

    def finish(self):
        self.zlib(10, hold=0)
        self.parts.append(bgzf_member(zlib.compress(b"", 6)[2:-4], b""))          # bgzip's end-of-file member
        return b"".join(self.parts)


def _freqs(tokens, len258="285"):
    lf, df = [0] * 286, [0] * 30
    lf[256] = 1
    for t in tokens:
        if t.__class__ is int:
            lf[t] += 1
        else:
            lf[284 if t[0] == 258 and len258 == "284+31" else LEN_SYM[t[0]][0]] += 1
            df[DIST_SYM[t[1]][0]] += 1
    return lf, df


def long_code_lengths(tokens, len258="285"):
    """Literal/length and distance code lengths up to 15 bits with the symbols in use -- the frequent ones last -- on the longest."""
    lf, df = _freqs(tokens, len258)
    out = []
    for f in (lf, df):
        order = [s for s in range(len(f)) if f[s] == 0] + sorted((s for s in range(len(f)) if f[s]), key=lambda s: f[s])
        out.append(inverted_lengths(order, len(f)))
    return out


def long_length_code_lengths(tokens):
    """Literals on codes of at most 10 bits; end-of-block and every length symbol on 15-bit codes."""
    lf, df = _freqs(tokens)
    lits = limited_lengths([lf[s] if s < 256 else 0 for s in range(286)], 9)
    used = [s for s in range(256) if lf[s]]
    order = [s for s in range(256) if not lf[s]] + list(range(256, 286))
    rest = inverted_lengths(order, 286, longest=14)
    lens = [(lits[s] + 1 if s in used else rest[s] + 1) for s in range(286)]
    return lens, limited_lengths(df, 15)


# ---------------------------------------------------------------------------------------------
# BGZF shapes
# ---------------------------------------------------------------------------------------------
def bgzf_long_codes(seed, pool):
    rng = random.Random(seed)
    F = BgzfFile(rng, pool)
    F.zlib(15)
    # long names that come back 17 KB later: lengths with 5 extra bits at distances with 13, on 15-bit codes both
    s = F.script()
    names = [name_of(rng, "long") for _ in range(56)]
    for i in range(150):
        F.rec(s, fixed_read(rng, pool, 50), names[i % len(names)], qual_of(rng, 50, "skewed"), farthest=True)
    ll, dl = long_code_lengths(s.tokens)
    F.crafted("frequent symbols on 15 bits, both codes", [Block("dynamic", s.tokens, lit_lens=ll, dist_lens=dl)], s.text)
    F.zlib(9)
    s = F.script()
    for i in range(60):
        F.rec(s, fixed_read(rng, pool, 40), name_of(rng, "plain", i), qual_of(rng, 40, "skewed"))
    ll, dl = long_length_code_lengths(s.tokens)
    F.crafted("only end-of-block and the lengths", [Block("dynamic", s.tokens, lit_lens=ll, dist_lens=dl)], s.text)
    return F


def bgzf_extremes(seed, pool):
    rng = random.Random(seed)
    F = BgzfFile(rng, pool)
    F.zlib(15, hold=0)
    s = F.script()                                            # (nothing pending: positions are the member's own)
    n0 = bytes(rng.choice(b"abcdefghijklmnopqrstuvwxyz0123456789") for _ in range(2500))
    s.lit(b"@" + n0 + b"\n")
    r = fixed_read(rng, pool, 60)
    F.reads.append(r)
    s.lit(r.encode() + b"\n+\n").lit(qual_of(rng, 60, "geometric") + b"\n")

    def special(make_name):
        """A record whose name is written by make_name(s) (copies and all)."""
        s.lit(b"@")
        make_name(s)
        s.lit(b"\n")
        r = fixed_read(rng, pool, 45)
        F.reads.append(r)
        s.lit(r.encode() + b"\n+\n")
        s.lit(b"I")
        s.copy(44, 1)                                         # distance 1
        s.lit(b"\n")

    def filler_to(target):
        """Records up to byte `target`: the next record's '@' lands there."""
        while target - s.pos > 400:
            F.rec(s, fixed_read(rng, pool, 45), name_of(rng, "plain", s.pos), None)
        gap = target - s.pos                                  # one record of exactly `gap` bytes: '@' name \n 45 \n+\n 45 \n
        name = bytes(rng.choice(b"xyzXYZ") for _ in range(gap - 1 - 1 - 45 - 3 - 45 - 1))
        F.rec(s, fixed_read(rng, pool, 45), name, qual_of(rng, 45, "skewed"))
        assert s.pos == target

    # every length symbol, at its base length (258 twice: both spellings come from the block's len258), from the first name
    for k, n in enumerate(LEN_BASE + [4, 258]):
        special(lambda s, n=n, k=k: s.copy(n, s.pos - 1 - (k % 7)))
    # a match that reaches byte 0 of the member: the distance equals the position
    special(lambda s: (s.text.pop(), s.tokens.pop(), s.copy(40, s.pos)))     # ('@' itself is copied from byte 0)
    # distance 2 with overlap, length 3 and 258
    special(lambda s: s.lit(b"ab").copy(3, 2).copy(258, 2))
    for dist, n, source in ((24577, 100, 50), (32767, 50, 50), (32768, 258, 600), (32768, 3, 1200), (32767, 3, 1800)):
        filler_to(dist + source - 1)                          # (the name begins one byte behind the '@')
        special(lambda s, dist=dist, n=n: s.copy(n, dist))
    half = len(s.tokens) // 2
    blocks = [Block("dynamic", s.tokens[:half], len258="284+31"), Block("fixed", s.tokens[half:half + 200], len258="284+31"),
              Block("dynamic", s.tokens[half + 200:])]
    F.crafted("extremes of the alphabets", blocks, s.text)
    # length 258 as 284 + 31 where it is FREQUENT: a short code, so the primary tables see it (above it is rare: a long code)
    F.zlib(3)
    s = F.script()
    for i in range(8):
        r = "ACGT"[i % 4] * (3 * 258 + 40 + i)
        F.reads.append(r)
        s.lit(b"@run %d\n" % i + r[:1].encode()).copy(258, 1).copy(258, 1).copy(258, 1).copy(39 + i, 1).lit(b"\n+\n")
        s.lit(b"I").copy(258, 1).copy(258, 1).copy(258, 1).copy(39 + i, 1).lit(b"\n")
    half = len(s.tokens) // 2
    F.crafted("length 258 as 284 + 31 on short codes", [Block("dynamic", s.tokens[:half], len258="284+31"), Block("fixed", s.tokens[half:], len258="284+31")], s.text)
    return F


def bgzf_overlap(seed, pool):
    rng = random.Random(seed)
    F = BgzfFile(rng, pool)
    F.zlib(15)
    s = F.script()
    for d in (1, 2, 3, 4, 5, 6, 7, 8, 9, 63, 64, 65) * 2:
        for n in (d + 1, d + 2, 2 * d + 3, 3 * d + 70):
            n = max(3, 30 - d, min(258, n))
            r = fixed_read(rng, pool, d + n)
            F.reads.append(r)
            s.auto(b"@" + name_of(rng, "any") + b"\n" + r.encode() + b"\n+\n")
            s.lit(qual_of(rng, d, "geometric")).copy(n, d).lit(b"\n")        # (the source begins in literals of the same batch)
    # chains: every match reads what the one before it wrote
    for d, n, count in ((5, 5, 260), (3, 3, 420), (5, 7, 205), (40, 6, 210), (1, 3, 300), (9, 7, 202)):
        length = d + n * count
        r = (gen.rand_seq(rng, d) * (length // d + 1))[:length]
        F.reads.append(r)
        s.lit(b"@chain %d %d\n" % (d, n))
        s.lit(r[:d].encode())
        for _ in range(count):
            s.copy(n, d)
        assert bytes(s.text[-length:]) == r.encode()
        s.lit(b"\n+\n")
        s.lit(qual_of(rng, d, "skewed"))
        for _ in range(count):
            s.copy(n, d)
        s.lit(b"\n")
    assert len(s.text) <= 65280
    F.crafted("overlap and chains", [Block("dynamic", s.tokens)], s.text)
    # the same chains through the fixed code (short codes: the most matches to a batch)
    F.zlib(5)
    s = F.script()
    r = (gen.rand_seq(rng, 4) * 600)[:4 + 3 * 500]
    F.reads.append(r)
    s.lit(b"@fixed chain\n" + r[:4].encode())
    for _ in range(500):
        s.copy(3, 4)
    s.lit(b"\n+\n" + b"IJKL")
    for _ in range(500):
        s.copy(3, 4)
    s.lit(b"\n")
    F.crafted("chains in one-bit codes", [Block("dynamic", s.tokens, lit_lens=_two_code_lengths(s.tokens), dist_lens=None)], s.text)
    return F


def _two_code_lengths(tokens):
    """The length symbol in use on one bit, everything else behind the other bit."""
    lf, _ = _freqs(tokens)
    hot = max(range(257, 286), key=lambda s: lf[s])
    rest = limited_lengths([0 if s == hot else lf[s] for s in range(286)], 14)
    return [1 if s == hot else (rest[s] + 1 if rest[s] else 0) for s in range(286)]


def bgzf_small_blocks(seed, pool):
    rng = random.Random(seed)
    F = BgzfFile(rng, pool)
    F.zlib(15)
    s = F.script()
    names = [name_of(rng, "long")[:60] for _ in range(8)]
    quals = [qual_of(rng, 44, "geometric") for _ in range(12)]
    while s.pos < 59000:
        q = bytearray(rng.choice(quals))
        q[rng.randrange(44)] = rng.randrange(33, 127)
        F.rec(s, fixed_read(rng, pool, 44), rng.choice(names) + b"%d" % rng.randrange(1000), bytes(q))
    tokens = s.tokens
    blocks, i, k = [], 0, 0
    text_at = 0
    text = bytes(s.text)
    want_end = 0
    while i < len(tokens):
        kind = ("stored", "fixed", "dynamic")[k % 3]
        n = rng.randrange(1, 41)
        if k % 17 == 3:
            n = 0                                             # stored blocks of length 0, empty fixed blocks, end-of-block-only dynamic ones
        part = tokens[i:i + n]
        i += n
        span = sum(1 if t.__class__ is int else t[0] for t in part)
        if kind == "stored":
            blocks.append(Block("stored", text[text_at:text_at + span]))
        elif kind == "fixed":
            blocks.append(Block("fixed", part))
        else:
            # (the block in front of a stored one: it ends at each bit offset in turn)
            # (a header too small to pad that far ends where it ends: the CPU tier asserts that all eight offsets occur)
            blocks.append(Block("dynamic", part, end_bit=want_end % 8, end_bit_or_nearest=True, header=("zlib", "plain", "cross")[k % 9 // 3]))
            want_end += 1
        text_at += span
        k += 1
    blocks.append(Block(("fixed", "dynamic", "stored")[seed % 3]))          # the final block is empty
    F.crafted("many small blocks", blocks, s.text)
    return F


def crossing_header_members(rng, pool, reads, new_script):
    """(name, script, block) of three dynamic blocks whose headers carry a 16, a 17 and an 18 that run from the literal/length
    lengths into the distance lengths.  new_script() starts each one's text; its reads are appended to `reads`."""

    def periodic(s, n_records, dists, fours=True):
        """Records whose quality lines are copies of length 3 (and 4) at the given distances."""
        for i in range(n_records):
            r = fixed_read(rng, pool, 40)
            reads.append(r)
            s.lit(b"@" + name_of(rng, "plain", i) + b"\n" + r.encode() + b"\n+\n")
            d = max(dists)
            s.lit(qual_of(rng, d, "skewed"))
            left = 40 - d                                     # 36: three of four and eight of three, or twelve of three
            lengths = [4, 4, 4] + [3] * 8 if fours else [3] * 12
            assert sum(lengths) == left
            for k, n in enumerate(lengths):
                s.copy(n, dists[k % len(dists)])
            s.lit(b"\n")

    # a 16 across the boundary: ... 257:2 258:2 | 2 2 2 2
    s = new_script()
    periodic(s, 12, (1, 2, 3, 4))
    lf, _ = _freqs(s.tokens)
    rest = limited_lengths([0 if x in (257, 258) else lf[x] for x in range(286)], 14)
    ll = [2 if x in (257, 258) else (rest[x] + 1 if rest[x] else 0) for x in range(286)]
    yield "header: 16 across the boundary", s, Block("dynamic", s.tokens, lit_lens=ll, dist_lens=[2, 2, 2, 2], header="cross")
    # a 17: 258 259 | 0 0 are zero, distances 3 and 4 on one bit each
    s = new_script()
    periodic(s, 12, (4, 3), fours=False)
    yield "header: 17 across the boundary", s, Block("dynamic", s.tokens, dist_lens=[0, 0, 1, 1], hlit=260, header="cross")
    # an 18: 259..285 and the first distance codes are zero
    s = new_script()
    far = [name_of(rng, "long") for _ in range(8)]
    for i in range(40):
        r = fixed_read(rng, pool, 40)
        reads.append(r)
        s.auto(record(far[i % 8], r, qual_of(rng, 40, "skewed")), min_len=100)
    yield "header: 18 across the boundary", s, Block("dynamic", s.tokens, hlit=286, header="cross")


def bgzf_headers(seed, pool):
    rng = random.Random(seed)
    F = BgzfFile(rng, pool)
    F.zlib(15)

    def literal_records(s, n, names, quals):
        for i in range(n):
            r = fixed_read(rng, pool, 40)
            F.reads.append(r)
            s.lit(record(name_of(rng, names, i), r, qual_of(rng, 40, quals)))

    # HLIT = 286, HDIST = 30, eight code-length codes (HCLEN field 4): 16 17 18 0 8 7 9 6 -- all a header can name then are
    # lengths 6..9 and 0 (a count of four would leave no length for the end-of-block code: no such block exists)
    s = F.script()
    literal_records(s, 30, "any", "geometric")
    lf, _ = _freqs(s.tokens)
    F.crafted("header: 286 / 30 / 8", [Block("dynamic", s.tokens, lit_lens=bounded_lengths(lf, 6, 9), dist_lens=[0] * 30, hlit=286, hdist=30, hclen=8)], s.text)
    F.zlib(4)
    s = F.script()
    for i in range(40):
        F.rec(s, fixed_read(rng, pool, 40), name_of(rng, "plain", i), qual_of(rng, 40, "skewed"))
    F.crafted("header: 286 / 30 / 19", [Block("dynamic", s.tokens, hlit=286, hdist=30, hclen=19, header="plain")], s.text)
    F.zlib(4)

    for name, s, block in crossing_header_members(rng, pool, F.reads, F.script):
        F.crafted(name, [block], s.text)
        F.zlib(3)
    # an 18 with 138 repeats: no byte above 'u' in the text
    s = F.script()
    literal_records(s, 25, "low", "low")
    s.lit(b"@u\nA\n+\nI\n")
    F.reads.append("A")
    F.crafted("header: an 18 with 138 repeats, no distance code", [Block("dynamic", s.tokens, header="zlib")], s.text)
    F.zlib(3)
    # one distance code of one bit
    s = F.script()
    for i in range(20):
        r = fixed_read(rng, pool, 40)
        F.reads.append(r)
        s.lit(b"@" + name_of(rng, "any") + b"\n" + r.encode() + b"\n+\n" + b"F").copy(39, 1).lit(b"\n")
    F.crafted("header: one distance code of one bit", [Block("dynamic", s.tokens)], s.text)
    return F


def bgzf_ring_edges(seed, pool):
    rng = random.Random(seed)
    F = BgzfFile(rng, pool)
    F.zlib(15)
    # payloads of 512 k + {0, 1, 7, 8} bytes: a fixed block whose last name (bytes below 144: eight bits each) is as long as it takes
    for extra in (0, 1, 7, 8):
        s = F.script()
        for i in range(20):
            F.rec(s, fixed_read(rng, pool, 40), name_of(rng, "plain", i), qual_of(rng, 40, "skewed"))
        base = len(deflate([Block("fixed", s.tokens, final=True)])[0])
        r = fixed_read(rng, pool, 40)
        tail = b"\n" + r.encode() + b"\n+\n" + qual_of(rng, 40, "skewed") + b"\n"
        fixed_part = len(deflate([Block("fixed", s.tokens + list(b"@" + tail), final=True)])[0]) - base
        grow = (-(base + fixed_part) + extra) % 512
        F.reads.append(r)
        s.lit(b"@" + bytes(rng.choice(b"abcdefghij") for _ in range(grow)) + tail)
        blocks = [Block("fixed", s.tokens)]
        raw = deflate([Block("fixed", s.tokens, final=True)])[0]
        assert len(raw) % 512 == extra, (len(raw), extra)
        F.crafted("payload of 512 k + %d bytes" % extra, blocks, s.text)
        F.zlib(3)
    # end-of-block on the last bit of the payload, and on its first
    for end_bit, what in ((0, "last"), (1, "first")):
        s = F.script()
        for i in range(30):
            F.rec(s, fixed_read(rng, pool, 40), name_of(rng, "any"), qual_of(rng, 40, "geometric"))
        F.crafted("end-of-block on the %s bit of the payload's last byte" % what, [Block("dynamic", s.tokens, end_bit=end_bit)], s.text)
        F.zlib(3)
    # wide symbols (15 + 5 + 15 + 13 bits) across the 512-byte boundaries of the payload
    s = F.script()
    names = [name_of(rng, "long") for _ in range(70)]
    for i in range(200):
        F.rec(s, fixed_read(rng, pool, 8 + 28), names[i % len(names)], qual_of(rng, 36, "skewed")[:36], farthest=True)
    ll, dl = long_code_lengths(s.tokens)
    F.crafted("wide symbols across the ring's halves", [Block("dynamic", s.tokens, lit_lens=ll, dist_lens=dl)], s.text)
    return F


def libdeflate_compress(data, level):
    """Raw DEFLATE by libdeflate (what htslib's bgzip links), or None where the library is not installed."""
    try:
        lib = ctypes.CDLL("libdeflate.so.0")
    except OSError:
        return None
    lib.libdeflate_alloc_compressor.restype = ctypes.c_void_p
    lib.libdeflate_alloc_compressor.argtypes = [ctypes.c_int]
    lib.libdeflate_deflate_compress.restype = ctypes.c_size_t
    lib.libdeflate_deflate_compress.argtypes = [ctypes.c_void_p, ctypes.c_char_p, ctypes.c_size_t, ctypes.c_char_p, ctypes.c_size_t]
    lib.libdeflate_free_compressor.argtypes = [ctypes.c_void_p]
    c = lib.libdeflate_alloc_compressor(level)
    if not c:
        return None
    out = ctypes.create_string_buffer(len(data) + 1024)
    n = lib.libdeflate_deflate_compress(c, data, len(data), out, len(out))
    lib.libdeflate_free_compressor(c)
    return out.raw[:n] if n else None


def bgzf_libdeflate(seed, pool):
    """None where libdeflate is not installed."""
    if libdeflate_compress(b"probe", 6) is None:
        return None
    rng = random.Random(seed)
    F = BgzfFile(rng, pool)
    F.zlib(15)
    for level in (1, 6, 12):
        for n, names, quals in ((200, "plain", "skewed"), (100, "long", "geometric"), (3, "any", "geometric")):
            data = F.pending + F.records(n, names=names, quals=quals)
            F.pending = b""
            assert len(data) < 65000
            raw = libdeflate_compress(data, level)
            assert zlib_says(raw) == data
            F.streams.append(("libdeflate level %d, %s names" % (level, names), raw, data, Features()))
            F.parts.append(bgzf_member(raw, data))
            F.zlib(3)
    return F


BGZF_GROUPS = {
    "long codes": bgzf_long_codes,
    "extremes": bgzf_extremes,
    "overlap and chains": bgzf_overlap,
    "many small blocks": bgzf_small_blocks,
    "header shapes": bgzf_headers,
    "ring and payload edges": bgzf_ring_edges,
    "libdeflate": bgzf_libdeflate,
}


def bgzf_invalid(kind, seed, pool):
    """(file bytes, stream) of a BGZF file with one member that no inflater accepts."""
    rng = random.Random(seed)
    F = BgzfFile(rng, pool)
    F.zlib(15, hold=0)
    crc_text = size = None
    s = F.script(check=False)
    for i in range(5):
        F.rec(s, fixed_read(rng, pool, 40), name_of(rng, "plain", i), qual_of(rng, 40, "skewed"))
    if kind == "distance beyond the start":
        s.lit(b"@")
        at = s.pos
        s.copy(20, s.pos + 1)                                 # one byte in front of the member
        s.lit(b"\nACGT\n+\nIIII\n")
        blocks = [Block("dynamic", s.tokens)]
        # the trailer's CRC-32 is that of what a decoder WOULD produce if it took the byte in front of the member -- the last
        # byte of the member before, a newline -- for text: only the distance check tells this member from a valid one
        crc_text = bytes(s.text[:at]) + b"\n" * 20 + bytes(s.text[at + 20:])
    else:                                                     # a fixed block with literal/length symbol 286
        # (behind it six zero bits and the five of distance code 0: a decoder that took 286 for one more length symbol, with
        # six extra bits like the four before it, would copy 323 bytes from distance 1 and carry on)
        s.lit(b"@name\nACGT\n+\nII")
        s.tokens += [("code", 286), ("bits", 0, 11)]
        s.lit(b"II\n")
        blocks = [Block("fixed", s.tokens)]
        size = len(s.text) + 323
    F.crafted(kind, blocks, s.text, valid=False, crc_text=crc_text, size=size)
    F.zlib(5, hold=0)
    return F


# ---------------------------------------------------------------------------------------------
# ordinary gzip: a text of 128-byte records whose names come back every 32 KiB
# ---------------------------------------------------------------------------------------------
RECORD = 128
PERIOD = 32768 // RECORD


class GzipText:
    """Records of 128 bytes: '@' + a run of 12 equal bytes + 40 name bytes + \\n, 35 bases, +, 35 qualities.  Record r's name
    line equals that of the record 256 places, 32 KiB, back: it is written as a copy at distance 32768 (and, inside the run,
    32767), which is a copy of a copy ... back to the file's first 32 KiB.  tokens[r] are the tokens of record r; a block
    that begins with record r therefore begins with markers for byte 0 of the window in front of it and onwards.  Four
    records are eight places (1024 bytes) long instead: 500 equal bases and 500 equal qualities, each a literal, a match of
    258 and one of 241 at distance 1 -- blocks alternate between the two spellings of 258."""
    LONG = (1000, 1021, 3003, 3050)

    def __init__(self, seed, pool, n_records=7168):
        rng = random.Random(seed)
        self.reads = []
        self.tokens = []
        self.starts = []
        heads = []
        for k in range(PERIOD):
            run = bytes([rng.choice(b"abcdefgh")]) * 12
            heads.append(b"@" + run + bytes(rng.choice(ANY_BYTE) for _ in range(40)) + b"\n")
        quals = [qual_of(rng, 35, "geometric") for _ in range(64)]
        seen = {}
        text = bytearray()
        ordinary = []                                         # per place of 128 bytes: does an ordinary record begin there
        for r in range(n_records):
            at = len(text)
            self.starts.append(at)
            place = at // RECORD
            if r in self.LONG:
                base = "ACGT"[r % 4]
                self.reads.append(base * 500)
                head = b"@long record %06d\n" % r
                toks = list(head) + [ord(base), (258, 1), (241, 1)] + list(b"\n+\n") + [ord("I"), (258, 1), (241, 1), 10]
                text += head + base.encode() * 500 + b"\n+\n" + b"I" * 500 + b"\n"
                assert len(text) == at + 8 * RECORD
                ordinary += [False] * 8
                self.tokens.append(toks)
                continue
            head = heads[place % PERIOD]
            if place < PERIOD or not ordinary[place - PERIOD]:
                toks = list(head[:2]) + [(11, 1)] + list(head[13:])           # the run: distance 1
            else:
                style = r % 3
                if style == 0:
                    toks = [(7, 32768), (3, 32767), (3, 1), (41, 32768)]      # byte 0 of the missing window first
                elif style == 1:
                    toks = list(head[:2]) + [(11, 1), (41, 32768)]             # ... or a literal, distance 1, then the window
                else:
                    toks = [(54, 32768)]
            ordinary.append(True)
            read = fixed_read(rng, pool, 35)
            self.reads.append(read)
            toks += list(read.encode() + b"\n+\n")
            q = quals[rng.randrange(64)] if rng.random() < 0.6 else qual_of(rng, 35, "geometric")
            back = seen.get(q)
            if back is not None and at + 92 - back <= 32768 and at + 92 - back >= 36:
                toks += [(36, at + 92 - back)]
            else:
                toks += list(q + b"\n")
            seen[q] = at + 92
            text += head + read.encode() + b"\n+\n" + q + b"\n"
            assert len(text) == at + RECORD
            self.tokens.append(toks)
        self.starts.append(len(text))
        self.text = bytes(text)

    def blocks(self, per_block=14, kinds=("dynamic",), first=None, last_kind="dynamic", **options):
        """Blocks of `per_block` records each (about 1 KB of compressed data at 14), kinds cycled."""
        out = []
        n = len(self.tokens)
        for k, a in enumerate(range(0, n, per_block)):
            kind = kinds[k % len(kinds)] if a + per_block < n else last_kind
            if k == 0 and first:
                kind = first
            toks = [t for r in range(a, min(n, a + per_block)) for t in self.tokens[r]]
            spell = ("285", "284+31")[k % 2]
            if kind == "stored":
                out.append(Block("stored", self.text[self.starts[a]:self.starts[min(n, a + per_block)]]))
            elif options.get("long_codes"):
                ll, dl = long_code_lengths(toks, spell)
                out.append(Block(kind, toks, lit_lens=ll, dist_lens=dl, len258=spell))
            else:
                out.append(Block(kind, toks, len258=spell))
        out[-1].final = True
        return out


def gzip_file(blocks, text, reads):
    raw, f = deflate(blocks)
    return gzip_member(raw, text), raw, f, text, reads


def gzip_cases(G, pool):
    """{name: (file bytes, raw stream, Features, intended text, reads)} over one GzipText."""
    cases = {}
    blocks = G.blocks(14)
    last = blocks.pop()                                       # (a final dynamic block small enough to begin inside the last chunk)
    cut = len(last.tokens) - len(G.tokens[-1])
    blocks += [Block("dynamic", last.tokens[:cut]), Block("dynamic", last.tokens[cut:], final=True)]
    cases["blocks of about 1 KB, chains through every chunk"] = gzip_file(blocks, G.text, G.reads)
    cases["stored blocks across chunk boundaries"] = gzip_file(G.blocks(30, kinds=("dynamic", "stored", "dynamic", "fixed")), G.text, G.reads)
    cases["long-code blocks"] = gzip_file(G.blocks(40, long_codes=True), G.text, G.reads)
    cases["one dynamic block"] = gzip_file(G.blocks(len(G.tokens)), G.text, G.reads)
    cases["fixed blocks only"] = gzip_file(G.blocks(14, kinds=("fixed",), last_kind="fixed"), G.text, G.reads)
    cases["stored blocks only"] = gzip_file(G.blocks(400, kinds=("stored",), last_kind="stored"), G.text, G.reads)
    # headers with a 16, a 17 and an 18 that cross from the literal/length lengths into the distance lengths, read in symbol mode
    rng = random.Random(31)
    reads, front, front_text = [], [], b""
    for name, s, block in crossing_header_members(rng, pool, reads, Script):
        front.append(block)
        front_text += bytes(s.text)
    cases["repeats across the boundary in the first headers"] = gzip_file(front + G.blocks(14), front_text + G.text, reads + G.reads)
    # a last chunk shorter than 80 bits: the same blocks, then a final fixed block that ends with a name as long as it takes
    # (bytes below 144 take eight bits each in the fixed code; the stream begins at byte 10 of the file, the chunks are 4 KB)
    blocks[-1].final = False
    tail = b"\nACGT\n+\nIIII\n"
    bits = cases["blocks of about 1 KB, chains through every chunk"][2].end_bitpos + 3 + 8 * (1 + len(tail)) + 7
    grow = (5 - (bits + 7) // 8) % 4096
    name = bytes(b"abcdefghij"[i % 10] for i in range(grow))
    case = gzip_file(blocks + [Block("fixed", list(b"@" + name + tail), final=True)], G.text + b"@" + name + tail, G.reads + ["ACGT"])
    assert len(case[1]) % 4096 == 5, len(case[1]) % 4096
    cases["a last chunk of 40 bits"] = case
    return cases


def gzip_two_members_reaching_back(G, seed, pool):
    """Two members; the second, 20 KB into its text, copies from one byte in front of itself -- the first member's last byte,
    which lies right there in the decoder's buffer."""
    rng = random.Random(seed)
    first = G.blocks(14)
    raw1, _ = deflate(first)
    s = Script(check=False)
    reads = []
    for i in range(160):
        r = fixed_read(rng, pool, 35)
        reads.append(r)
        s.lit(record(name_of(rng, "any"), r, qual_of(rng, 35, "geometric")))
    s.lit(b"@")
    at = s.pos
    s.copy(30, s.pos + 1)
    s.lit(b"\nACGT\n+\nIIII\n")
    toks = s.tokens
    blocks = [Block("dynamic", toks[a:a + 1500]) for a in range(0, len(toks), 1500)]
    blocks[-1].final = True
    raw2, f = deflate(blocks)
    assert zlib_says(raw2) is None and len(raw2) > 3 * 4096
    # CRC-32 and size of what a decoder WOULD produce if it took the byte in front of the member for text: only the rule
    # that nothing in front of a member is text tells this file from a valid one
    would_be = bytes(s.text[:at]) + G.text[-1:] * 30 + bytes(s.text[at + 30:])
    assert len(would_be) == len(s.text)
    return gzip_member(raw1, G.text) + gzip_member(raw2, would_be), raw2, f
