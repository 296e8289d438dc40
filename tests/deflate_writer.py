"""A DEFLATE (RFC 1951) encoder that writes what a test says, not what compresses best: block types, code lengths,
header spelling, the spelling of length 258 and the bit offset a block ends at are all the caller's choice, and every
stream comes with a record of what was actually emitted (`Features`).  Standard library only.

    blocks = [Block("dynamic", tokens, lit_lens=..., header="cross"), Block("stored", tokens), Block("fixed", [], final=True)]
    raw, features = deflate(blocks)

A token is a literal byte (an int) or a match `(length, distance)`; `("code", s)` emits the bare literal/length code of
symbol `s` and `("bits", value, n)` n plain bits (for streams that are meant to be invalid).  `Script` builds a text and its tokens together, `tokenize` is a
simple matcher with knobs, `bgzf_member` / `gzip_member` wrap a stream like gen.write_bgzf and gzip do."""
import heapq
import struct
import zlib

LEN_BASE = [3, 4, 5, 6, 7, 8, 9, 10, 11, 13, 15, 17, 19, 23, 27, 31, 35, 43, 51, 59, 67, 83, 99, 115, 131, 163, 195, 227, 258]
LEN_EXTRA = [0, 0, 0, 0, 0, 0, 0, 0, 1, 1, 1, 1, 2, 2, 2, 2, 3, 3, 3, 3, 4, 4, 4, 4, 5, 5, 5, 5, 0]
DIST_BASE = [1, 2, 3, 4, 5, 7, 9, 13, 17, 25, 33, 49, 65, 97, 129, 193, 257, 385, 513, 769, 1025, 1537, 2049, 3073, 4097, 6145,
             8193, 12289, 16385, 24577]
DIST_EXTRA = [0, 0, 0, 0, 1, 1, 2, 2, 3, 3, 4, 4, 5, 5, 6, 6, 7, 7, 8, 8, 9, 9, 10, 10, 11, 11, 12, 12, 13, 13]
CL_ORDER = [16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15]
FIXED_LIT = [8] * 144 + [9] * 112 + [7] * 24 + [8] * 8
FIXED_DIST = [5] * 32


def _length_table():
    t = [None] * 259
    for s in range(28):
        for e in range(1 << LEN_EXTRA[s]):
            if LEN_BASE[s] + e <= 257:
                t[LEN_BASE[s] + e] = (257 + s, LEN_EXTRA[s], e)
    t[258] = (285, 0, 0)
    return t


def _dist_table():
    t = [None] * 32769
    for s in range(30):
        for e in range(1 << DIST_EXTRA[s]):
            t[DIST_BASE[s] + e] = (s, DIST_EXTRA[s], e)
    return t


LEN_SYM = _length_table()
DIST_SYM = _dist_table()


# ---------------------------------------------------------------------------------------------
# Huffman codes
# ---------------------------------------------------------------------------------------------
def kraft(lens, unit=15):
    """Sum of 2^-len over the codes, in units of 2^-unit: a complete set gives 1 << unit."""
    return sum(1 << (unit - l) for l in lens if l)


def check_lengths(lens, what="code"):
    """zlib's rule: complete, or a single code of one bit, or no code at all."""
    used = [l for l in lens if l]
    if not used or used == [1]:
        return
    k = kraft(lens)
    if k != 1 << 15:
        raise ValueError(f"{what}: code lengths are {'over-subscribed' if k > 1 << 15 else 'incomplete'} ({k} / 32768)")


def canonical_codes(lens):
    """{symbol: (code with its first bit in bit 0, length)} of the canonical code with these lengths."""
    codes, code, last = {}, 0, 0
    for l, s in sorted((l, s) for s, l in enumerate(lens) if l):
        code <<= l - last
        last = l
        codes[s] = (int(format(code, "0%db" % l)[::-1], 2), l)
        code += 1
    return codes


def limited_lengths(freqs, limit=15):
    """Huffman code lengths for the symbols of non-zero frequency, none longer than `limit`; complete unless only one symbol
    is used (that one gets one bit, as zlib accepts)."""
    lens = [0] * len(freqs)
    used = [s for s, f in enumerate(freqs) if f > 0]
    if not used:
        return lens
    if len(used) == 1:
        lens[used[0]] = 1
        return lens
    heap = [(freqs[s], s, (s,)) for s in used]
    heapq.heapify(heap)
    tick = len(freqs)
    while len(heap) > 1:
        fa, _, a = heapq.heappop(heap)
        fb, _, b = heapq.heappop(heap)
        for s in a + b:
            lens[s] += 1
        heapq.heappush(heap, (fa + fb, tick, a + b))
        tick += 1
    if max(lens) > limit:
        for s in used:
            lens[s] = min(lens[s], limit)
        full = 1 << limit
        k = kraft(lens, limit)
        order = sorted(used, key=lambda s: (-lens[s], freqs[s]))             # longest and rarest first
        while k > full:
            for s in order:
                if lens[s] < limit:
                    lens[s] += 1
                    k -= 1 << (limit - lens[s])
                    break
            order.sort(key=lambda s: (-lens[s], freqs[s]))
        for s in sorted(used, key=lambda s: -freqs[s]):                      # hand the slack to the frequent ones
            while lens[s] > 1 and k + (1 << (limit - lens[s])) <= full:
                k += 1 << (limit - lens[s])
                lens[s] -= 1
        if k != full:
            raise ValueError("could not build a complete length-limited code")
    return lens


def inverted_lengths(order, n, longest=15):
    """A complete code over `order` (symbols, those to get the SHORT codes first) in an alphabet of n: everything starts at
    `longest` bits and the front of `order` is shortened until the set is complete -- the symbols at the back of `order`,
    the frequent ones if the caller says so, keep the longest codes."""
    lens = [0] * n
    for s in order:
        lens[s] = longest
    full, k = 1 << longest, len(order)
    if k > full:
        raise ValueError("too many symbols")
    for s in order:
        while lens[s] > 1 and k + (1 << (longest - lens[s])) <= full:
            k += 1 << (longest - lens[s])
            lens[s] -= 1
        if k == full:
            break
    if len(order) > 1 and k != full:
        raise ValueError("incomplete")
    return lens


def bounded_lengths(freqs, lo, hi):
    """A complete code whose lengths all lie in [lo, hi] (for headers that may only name a few code lengths)."""
    used = sorted((s for s, f in enumerate(freqs) if f > 0), key=lambda s: -freqs[s])
    if not (1 << lo) <= len(used) <= (1 << hi):
        raise ValueError(f"{len(used)} symbols do not fit lengths {lo}..{hi}")
    lens = [0] * len(freqs)
    for s in used:
        lens[s] = hi
    full, k = 1 << hi, len(used)
    while k != full:
        moved = False
        for s in used:
            if lens[s] > lo and k + (1 << (hi - lens[s])) <= full:
                k += 1 << (hi - lens[s])
                lens[s] -= 1
                moved = True
        if not moved:
            raise ValueError("incomplete")
    return lens


# ---------------------------------------------------------------------------------------------
# bits
# ---------------------------------------------------------------------------------------------
class BitWriter:
    def __init__(self):
        self.out = bytearray()
        self.acc = 0
        self.n = 0

    def bits(self, v, k):
        self.acc |= v << self.n
        self.n += k
        if self.n >= 8192:
            self.spill()

    def spill(self):
        nb = self.n >> 3
        self.out += (self.acc & ((1 << (8 * nb)) - 1)).to_bytes(nb, "little")
        self.acc >>= 8 * nb
        self.n &= 7

    @property
    def bitpos(self):
        return len(self.out) * 8 + self.n

    def align(self):
        self.spill()
        if self.n:
            self.out.append(self.acc)
            self.acc = self.n = 0

    def done(self):
        self.align()
        return bytes(self.out)


class Block:
    """One DEFLATE block.  kind: "stored", "fixed", "dynamic".  For dynamic blocks:
    lit_lens / dist_lens  explicit code lengths (default: Huffman codes of the block's own tokens, at most max_bits long)
    check                 refuse incomplete / over-subscribed explicit lengths (switch off for streams meant to be invalid)
    header                "plain" (no repeats), "zlib" (repeats within each tree), "cross" (repeats over the joined lengths)
    hlit / hdist / hclen  the counts the header announces (padded with zero lengths): None = the smallest that will do
    len258                "285" or "284+31"
    end_bit               the block ends at this bit offset of a byte (0 = on a byte boundary), by padding the header
    end_bit_or_nearest    a header too small to be padded that far is written unpadded (default: that is an error)"""

    def __init__(self, kind, tokens=(), final=False, lit_lens=None, dist_lens=None, max_bits=15, check=True, header="zlib",
                 hlit=None, hdist=None, hclen=None, len258="285", end_bit=None, end_bit_or_nearest=False):
        self.kind, self.tokens, self.final = kind, list(tokens), final
        self.lit_lens, self.dist_lens, self.max_bits, self.check = lit_lens, dist_lens, max_bits, check
        self.header, self.hlit, self.hdist, self.hclen, self.len258, self.end_bit = header, hlit, hdist, hclen, len258, end_bit
        self.end_bit_or_nearest = end_bit_or_nearest


class Features:
    """What a stream really contains."""

    def __init__(self):
        self.max_lit_code = 0             # longest literal/length code emitted
        self.max_dist_code = 0            # longest distance code emitted
        self.long_pair_blocks = 0         # blocks that used a literal/length code > 10 bits AND a distance code > 8 bits
        self.long_length_only_blocks = 0  # blocks whose literals all have codes <= 10 bits, end-of-block and lengths longer ones
        self.lengths = set()
        self.length_symbols = set()
        self.distances = set()
        self.spell258 = set()
        self.blocks = {"stored": 0, "fixed": 0, "dynamic": 0}
        self.empty_blocks = {"stored": 0, "fixed": 0, "dynamic": 0}
        self.eob_only_dynamic = 0         # dynamic blocks whose only code is a one-bit end-of-block
        self.header_styles = set()
        self.crossing_repeats = set()     # 16 / 17 / 18 whose run covers lengths of both trees
        self.longest_18 = 0
        self.hlit, self.hdist, self.hclen = set(), set(), set()
        self.no_distance_code = 0         # dynamic blocks with HDIST = 1 and that length 0
        self.one_bit_distance_code = 0    # dynamic blocks with a single distance code
        self.eob_offsets = []             # bit offset (mod 8) behind every block
        self.block_starts = []            # bit position of every block's first header bit
        self.eob_before_stored = set()    # ... of the blocks a stored block follows
        self.wide_symbols_over_512 = 0    # matches of >= 40 bits that straddle a multiple of 512 bytes
        self.full_width_over_512 = 0      # ... of 48 bits (15 + 5 + 15 + 13)
        self.overlap_distances = set()    # distances of matches with dist < len
        self.longest_match_chain = 0      # most matches in a row, each reading bytes the match before it wrote
        self.reach_start = 0              # matches whose distance equals their position
        self.matches = 0
        self.literals = 0
        self.n_bytes = 0
        self.end_bitpos = 0

    def merge(self, other):
        for k, v in vars(other).items():
            mine = getattr(self, k)
            if isinstance(v, set):
                mine |= v
            elif isinstance(v, dict):
                for kk, vv in v.items():
                    mine[kk] += vv
            elif isinstance(v, list):
                mine.extend(v)
            elif k.startswith("max_") or k.startswith("longest_"):
                setattr(self, k, max(mine, v))
            else:
                setattr(self, k, mine + v)
        return self


def _rle(seq, style, hlit):
    """The code-length symbols for `seq`: [(symbol, extra value, extra bits, first index, count)]."""
    out = []
    spans = [(0, len(seq))] if style == "cross" else [(0, hlit), (hlit, len(seq))]
    for a, b in spans:
        i = a
        while i < b:
            v = seq[i]
            if style == "plain":
                out.append((v, 0, 0, i, 1))
                i += 1
                continue
            j = i
            while j < b and seq[j] == v:
                j += 1
            run = j - i
            if v == 0:
                while run >= 11:
                    r = min(run, 138)
                    out.append((18, r - 11, 7, i, r))
                    i += r
                    run -= r
                if run >= 3:
                    out.append((17, run - 3, 3, i, run))
                    i += run
                    run = 0
            else:
                out.append((v, 0, 0, i, 1))
                i += 1
                run -= 1
                while run >= 3:
                    r = min(run, 6)
                    out.append((16, r - 3, 2, i, r))
                    i += r
                    run -= r
            for _ in range(run):
                out.append((v, 0, 0, i, 1))
                i += 1
    return out


def _dynamic_header(b, lit_lens, dist_lens):
    """(value, bits) pieces of the header behind BFINAL / BTYPE, plus what it says about itself."""
    ll, dl = list(lit_lens), list(dist_lens)
    while len(ll) > 257 and ll[-1] == 0:
        ll.pop()
    while len(dl) > 1 and dl[-1] == 0:
        dl.pop()
    hlit = b.hlit if b.hlit is not None else len(ll)
    hdist = b.hdist if b.hdist is not None else len(dl)
    if hlit < len(ll) or hdist < len(dl):
        raise ValueError("hlit / hdist smaller than the codes in use")
    ll += [0] * (hlit - len(ll))
    dl += [0] * (hdist - len(dl))
    seq = ll + dl
    rle = _rle(seq, b.header, hlit)
    freq = [0] * 19
    for s, *_ in rle:
        freq[s] += 1
    if sum(1 for f in freq if f) < 2:                     # the code-length code must be complete: two codes at least
        freq[0 if freq[0] == 0 else 18] += 1
    cl = limited_lengths(freq, 7)
    n = 19
    while n > 4 and cl[CL_ORDER[n - 1]] == 0:
        n -= 1
    hclen = b.hclen if b.hclen is not None else n
    if hclen < n:
        raise ValueError(f"hclen {hclen} does not reach the code lengths in use ({n})")
    codes = canonical_codes(cl)
    pieces = [(hlit - 257, 5), (hdist - 1, 5), (hclen - 4, 4)] + [(cl[CL_ORDER[i]], 3) for i in range(hclen)]
    crossing, longest18 = set(), 0
    for s, ev, eb, at, cnt in rle:
        pieces.append(codes[s])
        if eb:
            pieces.append((ev, eb))
        if s >= 16 and at < hlit < at + cnt:
            crossing.add(s)
        if s == 18:
            longest18 = max(longest18, cnt)
    return pieces, (hlit, hdist, hclen, n, crossing, longest18)


_FIXED_CODES = (canonical_codes(FIXED_LIT), canonical_codes(FIXED_DIST))


def deflate(blocks, features=None):
    """The raw DEFLATE stream of `blocks` and its Features."""
    f = features or Features()
    w = BitWriter()
    pos = 0                                                  # bytes of text so far
    prev_end = None
    for b in blocks:
        f.block_starts.append(w.bitpos)
        f.blocks[b.kind] += 1
        if not b.tokens:
            f.empty_blocks[b.kind] += 1
        if b.kind == "stored":
            if prev_end is not None:
                f.eob_before_stored.add(prev_end)
            data = bytes(b.tokens)
            if len(data) > 65535:
                raise ValueError("a stored block holds at most 65535 bytes")
            w.bits(1 if b.final else 0, 1)
            w.bits(0, 2)
            w.align()
            w.out += struct.pack("<HH", len(data), len(data) ^ 0xFFFF) + data
            pos += len(data)
            f.literals += len(data)
            prev_end = 0
            f.eob_offsets.append(0)
            continue
        toks = b.tokens
        if b.kind == "fixed":
            lit_lens, dist_lens = FIXED_LIT, FIXED_DIST
        else:
            lit_lens, dist_lens = b.lit_lens, b.dist_lens
            if lit_lens is None or dist_lens is None:
                lf, df = [0] * 286, [0] * 30
                lf[256] = 1
                for t in toks:
                    if t.__class__ is int:
                        lf[t] += 1
                    elif t[0] == "code":
                        lf[t[1]] += 1
                    else:
                        lf[284 if t[0] == 258 and b.len258 == "284+31" else LEN_SYM[t[0]][0]] += 1
                        df[DIST_SYM[t[1]][0]] += 1
                if lit_lens is None:
                    lit_lens = limited_lengths(lf, b.max_bits)
                if dist_lens is None:
                    dist_lens = limited_lengths(df, b.max_bits)
            if b.check:
                check_lengths(lit_lens, "literal/length")
                check_lengths(dist_lens, "distance")
        lc, dc = (_FIXED_CODES if b.kind == "fixed" else (canonical_codes(lit_lens), canonical_codes(dist_lens)))
        w.bits(1 if b.final else 0, 1)
        w.bits(1 if b.kind == "fixed" else 2, 2)
        if b.kind == "dynamic":
            pieces, (hlit, hdist, hclen, n_cl, crossing, longest18) = _dynamic_header(b, lit_lens, dist_lens)
            if b.end_bit is not None:
                # the body's size does not depend on the header's: pad HCLEN (3 bits a step) until the block ends where it should
                body = lc[256][1]
                for t in toks:
                    if t.__class__ is int:
                        body += lc[t][1]
                    elif t[0] == "code":
                        body += lc[t[1]][1]
                    else:
                        ls, eb, _ = (284, 5, 31) if t[0] == 258 and b.len258 == "284+31" else LEN_SYM[t[0]]
                        ds, deb, _ = DIST_SYM[t[1]]
                        body += lc[ls][1] + eb + dc[ds][1] + deb
                ll_n = max([257] + [i + 1 for i, l in enumerate(lit_lens) if l])
                dl_n = max([1] + [i + 1 for i, l in enumerate(dist_lens) if l])
                trials = [(hl, hd, extra) for hl in range(b.hlit or ll_n, min(286, (b.hlit or ll_n) + 9) + 1)
                          for hd in range(b.hdist or dl_n, min(30, (b.hdist or dl_n) + 3) + 1) for extra in range(8)]
                for hl, hd, extra in trials:
                    trial = Block("dynamic", hlit=hl, hdist=hd, header=b.header)
                    n_here = _dynamic_header(trial, lit_lens, dist_lens)[1][3]
                    if n_here + extra > 19:
                        continue
                    trial.hclen = n_here + extra
                    pieces, (hlit, hdist, hclen, _, crossing, longest18) = _dynamic_header(trial, lit_lens, dist_lens)
                    if (w.bitpos + sum(k for _, k in pieces) + body) % 8 == b.end_bit:
                        break
                else:
                    if not b.end_bit_or_nearest:
                        raise ValueError(f"no header padding ends this block at bit {b.end_bit}")
                    pieces, (hlit, hdist, hclen, n_cl, crossing, longest18) = _dynamic_header(b, lit_lens, dist_lens)
            for v, k in pieces:
                w.bits(v, k)
            f.header_styles.add(b.header)
            f.crossing_repeats |= crossing
            f.longest_18 = max(f.longest_18, longest18)
            f.hlit.add(hlit)
            f.hdist.add(hdist)
            f.hclen.add(hclen)
            used_d = [l for l in dist_lens if l]
            if hdist == 1 and not used_d:
                f.no_distance_code += 1
            if used_d == [1]:
                f.one_bit_distance_code += 1
            if [l for l in lit_lens if l] == [1] and lit_lens[256] == 1:
                f.eob_only_dynamic += 1
        max_l = max_d = max_literal = 0
        min_len_code = 99
        # (literals, the bulk of any stream, go through local copies of the writer's accumulator)
        acc, nb, n_lit = w.acc, w.n, 0
        chain, prev_a, prev_b = 0, 0, 0                      # the run of matches so far, the text range the last one wrote
        for t in toks:
            if t.__class__ is int:
                c = lc[t]
                acc |= c[0] << nb
                nb += c[1]
                if c[1] > max_literal:
                    max_literal = c[1]
                n_lit += 1
                if nb >= 4096:
                    w.acc, w.n = acc, nb
                    w.spill()
                    acc, nb = w.acc, w.n
                continue
            w.acc, w.n = acc, nb
            if t[0] == "code":
                c = lc[t[1]]
                w.bits(c[0], c[1])
                acc, nb = w.acc, w.n
                continue
            if t[0] == "bits":
                w.bits(t[1], t[2])
                acc, nb = w.acc, w.n
                continue
            n, d = t
            at0 = w.bitpos
            if n == 258 and b.len258 == "284+31":
                ls, eb, ev = 284, 5, 31
                f.spell258.add("284+31")
            else:
                ls, eb, ev = LEN_SYM[n]
                if n == 258:
                    f.spell258.add("285")
            c = lc[ls]
            w.bits(c[0], c[1])
            if eb:
                w.bits(ev, eb)
            max_l = max(max_l, c[1])
            min_len_code = min(min_len_code, c[1])
            ds, deb, dev = DIST_SYM[d]
            c = dc[ds]
            w.bits(c[0], c[1])
            if deb:
                w.bits(dev, deb)
            max_d = max(max_d, c[1])
            at1 = w.bitpos
            if at1 - at0 >= 40 and (at0 >> 12) != ((at1 - 1) >> 12):
                f.wide_symbols_over_512 += 1
                if at1 - at0 == 48:
                    f.full_width_over_512 += 1
            here = pos + n_lit
            if d < n:
                f.overlap_distances.add(d)
            chain = chain + 1 if (chain and not n_lit and here - d < prev_b and here - d + min(n, d) > prev_a) else 1
            prev_a, prev_b = here, here + n
            if chain > f.longest_match_chain:
                f.longest_match_chain = chain
            f.lengths.add(n)
            f.length_symbols.add(ls)
            f.distances.add(d)
            f.matches += 1
            if d == pos + n_lit:
                f.reach_start += 1
            pos += n + n_lit
            f.literals += n_lit
            n_lit = 0
            acc, nb = w.acc, w.n
        w.acc, w.n = acc, nb
        pos += n_lit
        f.literals += n_lit
        c = lc[256]
        w.bits(c[0], c[1])
        f.max_lit_code = max(f.max_lit_code, max_l, max_literal, c[1])
        f.max_dist_code = max(f.max_dist_code, max_d)
        if max(max_l, max_literal) > 10 and max_d > 8:
            f.long_pair_blocks += 1
        if max_literal <= 10 and c[1] > 10 and min_len_code != 99 and min_len_code > 10:
            f.long_length_only_blocks += 1
        prev_end = w.bitpos % 8
        f.eob_offsets.append(prev_end)
    f.n_bytes = pos
    f.end_bitpos = w.bitpos                                  # (before the last byte is padded)
    return w.done(), f


# ---------------------------------------------------------------------------------------------
# text and tokens
# ---------------------------------------------------------------------------------------------
def expand(tokens, check=True):
    """The text a token list stands for (None when a distance reaches in front of it and check is off)."""
    out = bytearray()
    for t in tokens:
        if t.__class__ is int:
            out.append(t)
        elif t[0] in ("code", "bits"):
            return None
        else:
            n, d = t
            if d > len(out):
                if check:
                    raise ValueError("distance beyond the start of the text")
                return None
            if d >= n:
                out += out[len(out) - d:len(out) - d + n]
            else:
                for _ in range(n):
                    out.append(out[-d])
    return bytes(out)


def tokenize(data, lo=0, hi=None, min_len=3, max_len=258, max_dist=32768, farthest=False, overlap=False, chain=24, heads=None):
    """Tokens for data[lo:hi], matches reaching back into data[:hi] (greedy, hash chains over 3-byte keys).
    farthest: among the candidates of the best length take the one farthest back (zlib takes the nearest);
    overlap:  a source closer than the match is long wins whenever there is one (dist < len);
    heads:    the chains of data[:lo] from an earlier call (they are extended)."""
    hi = len(data) if hi is None else hi
    if heads is None:
        heads = {}
        for i in range(max(0, lo - max_dist), lo):
            heads.setdefault(data[i:i + 3], []).append(i)
    out = []
    i = lo
    while i < hi:
        best_n, best_d = 0, 0
        key = data[i:i + 3]
        if i + min_len <= hi and len(key) == 3:
            cands = [j for j in heads.get(key, ()) if i - j <= max_dist]
            cands = cands[:chain] if farthest else cands[-chain:][::-1]
            limit = min(max_len, hi - i)
            for j in cands:
                n = 3
                while n + 16 <= limit and data[j + n:j + n + 16] == data[i + n:i + n + 16]:
                    n += 16
                while n < limit and data[j + n] == data[i + n]:
                    n += 1
                d = i - j
                better = n > best_n or (n == best_n and farthest and d > best_d)
                if overlap and best_n >= min_len:
                    better = (d < n) > (best_d < best_n) or ((d < n) == (best_d < best_n) and better)
                if n >= min_len and better:
                    best_n, best_d = n, d
        if best_n >= min_len:
            out.append((best_n, best_d))
            step = best_n
        else:
            out.append(data[i])
            step = 1
        for k in range(i, i + step):
            at = heads.setdefault(data[k:k + 3], [])
            at.append(k)
            if len(at) > 4 * chain:                           # (the oldest and the newest are what the knobs choose between)
                del at[chain:-chain]
        i += step
    return out


class Script:
    """A text written token by token: what a copy produces is whatever lies `dist` back."""

    def __init__(self, check=True):
        self.text = bytearray()
        self.tokens = []
        self.check = check
        self._heads, self._hashed = {}, 0

    @property
    def pos(self):
        return len(self.text)

    def lit(self, data):
        self.text += data
        self.tokens.extend(data)
        return self

    def copy(self, n, dist):
        if dist > len(self.text):
            if self.check:
                raise ValueError("distance beyond the start of the text")
            self.text += b"?" * n
        else:
            for _ in range(n):
                self.text.append(self.text[-dist])
        self.tokens.append((n, dist))
        return self

    def auto(self, data, **knobs):
        lo = len(self.text)
        for k in range(self._hashed, lo):                     # (what lit() and copy() wrote since)
            self._heads.setdefault(bytes(self.text[k:k + 3]), []).append(k)
        self.text += data
        self.tokens.extend(tokenize(bytes(self.text), lo, heads=self._heads, **knobs))
        self._hashed = len(self.text)
        return self


# ---------------------------------------------------------------------------------------------
# containers
# ---------------------------------------------------------------------------------------------
def bgzf_member(raw, text):
    """One BGZF member around a raw stream (the layout of gen.write_bgzf); CRC-32 and size are those of the intended text."""
    bsize = 12 + 6 + len(raw) + 8
    if bsize > 65536:
        raise ValueError(f"a BGZF member holds at most 64 KiB ({bsize})")
    head = b"\x1f\x8b\x08\x04" + b"\x00\x00\x00\x00" + b"\x00\xff" + struct.pack("<H", 6) + b"BC" + struct.pack("<HH", 2, bsize - 1)
    return head + raw + struct.pack("<II", zlib.crc32(text) & 0xFFFFFFFF, len(text) & 0xFFFFFFFF)


def gzip_member(raw, text):
    """One plain gzip member (no name, no extra field) around a raw stream."""
    return b"\x1f\x8b\x08\x00\x00\x00\x00\x00\x00\xff" + raw + struct.pack("<II", zlib.crc32(text) & 0xFFFFFFFF, len(text) & 0xFFFFFFFF)


def zlib_says(raw):
    """zlib's verdict on a raw stream: the text, or None when it raises / does not end with the input."""
    d = zlib.decompressobj(-15)
    try:
        out = d.decompress(raw)
    except zlib.error:
        return None
    return out if d.eof and not d.unused_data else None
