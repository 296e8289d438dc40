// scg_inflate.h -- the DEFLATE (RFC 1951) rules of the device decoders, and the decoder that walks one gzip member
// with a whole wavefront.
//
// BGZF files ("blocked gzip", what bgzip writes) are a concatenation of small independent gzip members (<= 64 KiB of
// text each) that announce their compressed size; the reference inflates them one after the other on the caller
// thread (byteme/GzipFileReader.hpp:39-51 -> zlib).  Here the compressed bytes cross the PCIe link as they are and
// every wavefront of scg_inflate.hip's kernels inflates one member (or one chunk of an ordinary gzip stream), its
// Huffman tables in LDS; the text never exists on the host.
//
// This is the project's ONE statement of the format's rules.  The host's chunk decoder (scg_pgzip.h), which takes the files
// the device's decoder hands back, has tables and a loop of its own, tuned for a host core, but takes every rule from
// here: a block header's limits, code-length code and repeat codes (read_code_lengths, for any bit reader), when a set of
// code lengths is a code (code_set_allowed), the fixed code (fixed_code_lengths), the bases and extra bits of length and
// distance symbols (length_* / dist_*), the markers.  (One exception, by measurement: the dynamic block filter, below.)
// The gzip container around the stream is scg_gzip.h's.
//
// The two device decoders share more -- the bit reader, the tables (fixed_tables, read_dynamic_tables), read_match and
// decode_here, a match's copy (copy_match):
//   * the lane-parallel decoder (scg_inflate.hip: inflate_lanes; the product's default, and stage 1 of the gzip path)
//     decodes 128 bit offsets at a time with decode_here and keeps only its scheduling -- batches, the chain walk,
//     deferred matches -- in the device file;
//   * inflate_member below (SCG_INFLATE_LANES=0: a measurement and test aid) walks the chain of dependent steps with
//     all lanes together: every value is wave-uniform, the compiler keeps the decoder's state in scalar registers, and
//     the lanes only differ where bytes move (a match is copied 64 bytes at a time, one per lane).
// Everything is plain C++, so the tests compile the very same code for the host (tests/inflate_harness.cpp:
// differential runs against zlib, corrupted streams under ASan): inflate_member with "wavefronts" of 1, 7 and 64
// lanes, a model of the lane-parallel decoder's arithmetic built from the same functions, and the host's chunk decoder
// beside them.  The CRC code's GF(2) arithmetic (gf2_mult, x_pow_bytes, at the end) lives here too, for the device's CRC
// kernel and the host side of the gzip path.
//
// Accept / reject behaviour follows zlib's inflate (inflate.c, inftrees.c) rule by rule -- over-subscribed and
// incomplete code sets, missing end-of-block code, too many length / distance symbols, invalid stored block lengths,
// distances beyond the start of the member -- because a member these decoders accept is not looked at by zlib again.
// Whatever they reject is redone by the host path, whose errors are zlib's own.  Every loop is bounded by the member's
// compressed and inflated sizes: a corrupt stream ends in an error, never in a runaway lane.
#ifndef SCG_INFLATE_H
#define SCG_INFLATE_H

#include <stdint.h>

#if defined(__HIPCC__)
#define SCG_HD __host__ __device__ inline __attribute__((always_inline))      // (__forceinline__, without the HIP runtime's header)
#else
#define SCG_HD inline
#endif

namespace scginf {

enum : int {
    INFLATE_OK = 0,
    INFLATE_BAD_DATA = 1,      // not a valid DEFLATE stream
    INFLATE_BAD_SIZE = 2,      // valid so far, but it does not fill / overruns the announced sizes
};

constexpr int LIT_BITS = 9, DIST_BITS = 7;                   // primary tables of the literal/length and the distance code: inflate_member
constexpr int LANES_LIT_BITS = 10, LANES_DIST_BITS = 8;      // the lane-parallel decoder (11 / 9 bits: no gain -- long codes are rare in FASTQ)
constexpr int CL_BITS = 7;                                   // the code-length code's longest code
constexpr int LENS_BYTES = 320 + 19;                         // a block header's code lengths, the code-length code's own behind them
constexpr uint32_t IN_SLACK = 64; // bytes readable beyond a member's payload (the caller pads its buffer)

// One block's tables (LDS on the device, one set per wavefront).
template<int LIT, int DIST>
struct Tables {
    static constexpr int lit_bits = LIT, dist_bits = DIST;
    uint16_t lit[1 << LIT];           // (code length << 12) | symbol, 0 = the code is longer than LIT bits (or invalid);
                                      // while a block header is read, the code lengths live here (bytes: 320 + 19 of them)
    uint16_t dtab[1 << DIST];         // the same for distance codes; during the header: the code-length code's table
    uint16_t lsym[288];               // literal/length symbols sorted by (code length, symbol)
    uint16_t dsym[32];
    uint16_t lcount[16];              // number of codes of each length
    uint16_t dcount[16];
    uint16_t offs[16];                // scratch of the table builder
};
typedef Tables<LIT_BITS, DIST_BITS> LaneTables;                   // 2016 bytes
typedef Tables<LANES_LIT_BITS, LANES_DIST_BITS> WaveTables;       // 3.3 KB

// The lanes that walk a member together ("Wave" below).  The decoder's own state is the same in every lane; the lanes
// differ only inside a Wave::Vec, a vector with one byte per lane, which the decoder moves around but never looks into:
//   width()                          lanes
//   set(v, j, byte)                  v[j] = byte
//   load(v, src, n, dist)            v[j] = src[j mod dist], j < n <= width()
//   store(dst, v, n)                 dst[j] = v[j], j < n
//   copy(dst, src, n, dist)          dst[j] = src[j mod dist], j < n, any n (src + dist <= dst: nothing it reads is written by it)
// On the device a Vec is one register and each operation one instruction per lane (scg_inflate.hip); the host tests
// run the same decoder with arrays (tests/inflate_harness.cpp), both one lane wide and 64 lanes wide.
template<int WIDTH>
struct HostWave {
    struct Vec { uint8_t b[WIDTH]; };
    SCG_HD uint32_t width() const { return WIDTH; }
    SCG_HD void set(Vec& v, uint32_t j, uint32_t byte) const { v.b[j] = static_cast<uint8_t>(byte); }
    SCG_HD void load(Vec& v, const uint8_t* src, uint32_t n, uint32_t dist) const { for (uint32_t j = 0; j < n; ++j) v.b[j] = src[j % dist]; }
    SCG_HD void store(uint8_t* dst, const Vec& v, uint32_t n) const { for (uint32_t j = 0; j < n; ++j) dst[j] = v.b[j]; }
    SCG_HD void copy(uint8_t* dst, const uint8_t* src, uint32_t n, uint32_t dist) const {
        // all loads of a round of WIDTH bytes before its stores, as the lanes of a wavefront do it
        for (uint32_t at = 0; at < n; at += WIDTH) {
            Vec v;
            const uint32_t m = n - at < static_cast<uint32_t>(WIDTH) ? n - at : static_cast<uint32_t>(WIDTH);
            for (uint32_t j = 0; j < m; ++j) v.b[j] = src[(at + j) % dist];
            for (uint32_t j = 0; j < m; ++j) dst[at + j] = v.b[j];
        }
    }
};

SCG_HD uint32_t load32(const uint8_t* p) { uint32_t v; __builtin_memcpy(&v, p, 4); return v; }
SCG_HD uint64_t load64(const uint8_t* p) { uint64_t v; __builtin_memcpy(&v, p, 8); return v; }
SCG_HD void store64(uint8_t* p, uint64_t v) { __builtin_memcpy(p, &v, 8); }

struct BitReader {
    const uint8_t* in;
    uint32_t pos;        // bytes of the stream that have entered buf
    uint32_t len;        // payload bytes; in[0 .. len + IN_SLACK) is readable
    uint64_t buf;        // LSB first
    uint32_t cnt;        // valid bits in buf
    uint32_t a0, a1;     // the stream's next two words, loaded ahead of their use: in[pos .. pos + 8)

    SCG_HD void open(const uint8_t* p, uint32_t n) {
        in = p; pos = 0; len = n; buf = 0; cnt = 0;
        a0 = load32(in);
        a1 = load32(in + 4);
    }
    // Stands at bit `bit` of the stream afterwards, with at least 33 bits in the buffer.
    SCG_HD void open_at_bit(const uint8_t* p, uint32_t n, uint32_t bit) {
        open(p, n);
        seek(bit >> 3);
        refill();
        bits(bit & 7u);
        refill();
    }
    // Continues at byte `at` of the stream (bit buffer empty).
    SCG_HD void seek(uint32_t at) {
        pos = at; buf = 0; cnt = 0;
        a0 = load32(in + pos);
        a1 = load32(in + pos + 4);
    }
    // At least 33 bits afterwards.  The word that enters the buffer was requested two refills ago.
    SCG_HD void refill() {
        if (cnt <= 32) {
            buf |= static_cast<uint64_t>(a0) << cnt;
            cnt += 32;
            pos += 4;
            a0 = a1;
            a1 = load32(in + pos + 4);
        }
    }
    SCG_HD uint32_t bits(uint32_t n) {
        const uint32_t v = static_cast<uint32_t>(buf) & ((1u << n) - 1u);
        buf >>= n;
        cnt -= n;
        return v;
    }
    SCG_HD uint32_t bit_position() const { return pos * 8u - cnt; }     // of the next unread bit
    SCG_HD bool overrun() const { return pos > len + 8; }     // more than the refill look-ahead beyond the payload
};

// The member's text.  Literals are collected, one per lane, and written a wavefront's width at a time.  A match of
// at most that many bytes is loaded at once but stored only when the next match comes along (or the text ends): the
// wavefront does not need the bytes to go on decoding, so the load's latency overlaps the next symbols.  Whatever reads
// text that is still pending -- a match whose source reaches into the pending literals or the pending match -- has it
// written out first.
template<class Wave>
struct TextWriter {
    const Wave& wave;
    uint8_t* out;
    uint32_t op;             // bytes produced
    uint32_t n_lit;          // of which the last n_lit are literals still in `lit`
    typename Wave::Vec lit;
    uint32_t m_at, m_n;      // a match of m_n bytes for out[m_at ...) still in `held`
    typename Wave::Vec held;

    SCG_HD TextWriter(const Wave& w, uint8_t* o) : wave(w), out(o), op(0), n_lit(0), m_at(0), m_n(0) {}
    SCG_HD void flush_literals() {
        if (n_lit) wave.store(out + op - n_lit, lit, n_lit);
        n_lit = 0;
    }
    SCG_HD void flush_match() {
        if (m_n) wave.store(out + m_at, held, m_n);
        m_n = 0;
    }
    SCG_HD void literal(uint32_t byte) {
        wave.set(lit, n_lit, byte);
        ++n_lit;
        ++op;
        if (n_lit == wave.width()) flush_literals();
    }
    // out[op + j] = out[op - dist + j mod dist], j < n; dist <= op.
    SCG_HD void match(uint32_t n, uint32_t dist) {
        const uint32_t src = op - dist, reach = src + (n < dist ? n : dist);      // reads out[src .. reach)
        flush_literals();                       // (pending literals are always the text's last bytes)
        if (m_n && reach > m_at && src < m_at + m_n) flush_match();
        if (n <= wave.width()) {
            typename Wave::Vec v;
            wave.load(v, out + src, n, dist);
            flush_match();                      // (the one before: its bytes have had a symbol or more to arrive)
            held = v;
            m_at = op;
            m_n = n;
        } else {
            flush_match();
            wave.copy(out + op, out + src, n, dist);
        }
        op += n;
    }
    // n bytes from elsewhere (a stored block)
    SCG_HD void raw(const uint8_t* from, uint32_t n) {
        flush_literals();
        flush_match();
        wave.copy(out + op, from, n, n ? n : 1u);
        op += n;
    }
    SCG_HD void finish() {
        flush_literals();
        flush_match();
    }
};

SCG_HD uint32_t reverse_bits(uint32_t code, int len) {
    uint32_t r = 0;
    for (int i = 0; i < len; ++i) { r = (r << 1) | (code & 1u); code >>= 1; }
    return r;
}

// Whether zlib takes a set of code lengths (inftrees.c: inflate_table), count[l] codes of length l = 1 .. 15, the longest
// of `max` >= 1 bits: never an over-subscribed set; an incomplete one only as a literal/length or distance code (kind 1)
// whose only code has one bit, and never as the code-length code (kind 0).
SCG_HD bool code_set_allowed(const uint16_t* count, int max, int kind) {
    int left = 1;
    for (int l = 1; l <= 15; ++l) {
        left <<= 1;
        left -= count[l];
        if (left < 0) return false;                           // over-subscribed
    }
    if (left > 0 && (kind == 0 || max != 1)) return false;    // incomplete
    return true;
}

// Builds the decoding tables of one canonical Huffman code from lens[0 .. n) (inftrees.c: inflate_table).
// kind: 0 = code-length code, 1 = literal/length or distance code (code_set_allowed).  Returns false for a set zlib rejects.
// `table` has 1 << tbits entries; `count`, `sym`, `offs` as in LaneTables.  lens may lie inside `table`: it is not read
// any more once the table is being written.
SCG_HD bool build_code(const uint8_t* lens, int n, int kind, uint16_t* table, int tbits, uint16_t* count, uint16_t* sym, uint16_t* offs) {
    for (int l = 0; l < 16; ++l) count[l] = 0;
    for (int s = 0; s < n; ++s) count[lens[s]] = static_cast<uint16_t>(count[lens[s]] + 1);
    int max = 15;
    while (max >= 1 && count[max] == 0) --max;
    if (max >= 1 && !code_set_allowed(count, max, kind)) return false;
    // (max == 0: no codes at all -- every lookup below fails, which is the error zlib raises when such a code is used)
    offs[1] = 0;
    for (int l = 1; l < 15; ++l) offs[l + 1] = static_cast<uint16_t>(offs[l] + count[l]);
    for (int s = 0; s < n; ++s) {
        const int l = lens[s];
        if (l) { sym[offs[l]] = static_cast<uint16_t>(s); offs[l] = static_cast<uint16_t>(offs[l] + 1); }
    }
    count[0] = 0;
    // lens is dead from here on
    for (int i = 0; i < (1 << tbits); ++i) table[i] = 0;
    uint32_t code = 0;
    int idx = 0;
    for (int l = 1; l <= tbits; ++l) {
        for (int k = 0; k < count[l]; ++k) {
            const uint16_t entry = static_cast<uint16_t>((l << 12) | sym[idx++]);
            for (uint32_t i = reverse_bits(code, l); i < (1u << tbits); i += 1u << l) table[i] = entry;
            ++code;
        }
        code <<= 1;
    }
    return true;
}

// A code that the primary table does not resolve: canonical decoding one bit at a time.  Returns the symbol, or -1
// for a bit pattern that is no code.  Needs 15 bits in the reader.
// A Reader (BitReader here, pgz::Bits on the host) has bits(n), refill(), overrun() and the fields buf (LSB first) and cnt;
// how far it may look beyond its input, and what overrun() therefore means, is its own buffer contract.
template<class Reader>
SCG_HD int decode_slow(Reader& br, const uint16_t* count, const uint16_t* sym) {
    uint32_t code = 0, first = 0, index = 0;
    uint32_t b = static_cast<uint32_t>(br.buf);
    for (int l = 1; l <= 15; ++l) {
        code |= b & 1u;
        b >>= 1;
        const uint32_t c = count[l];
        if (code < first + c) {
            br.buf >>= l;
            br.cnt -= static_cast<uint32_t>(l);
            return sym[index + (code - first)];
        }
        index += c;
        first = (first + c) << 1;
        code <<= 1;
    }
    return -1;
}

template<class Reader>
SCG_HD int decode_symbol(Reader& br, const uint16_t* table, int tbits, const uint16_t* count, const uint16_t* sym) {
    const uint32_t e = table[static_cast<uint32_t>(br.buf) & ((1u << tbits) - 1u)];
    if (e) {
        const uint32_t l = e >> 12;
        br.buf >>= l;
        br.cnt -= l;
        return static_cast<int>(e & 0xFFFu);
    }
    return decode_slow(br, count, sym);
}

// Length symbol 257 + t, t <= 28: its extra bits and its base; distance symbol d <= 29 likewise.
SCG_HD uint32_t length_extra(uint32_t t) { return (t < 8u || t == 28u) ? 0u : (t - 4u) >> 2; }
SCG_HD uint32_t length_base(uint32_t t, uint32_t eb) { return t < 8u ? t + 3u : (t == 28u ? 258u : ((4u + (t & 3u)) << eb) + 3u); }
SCG_HD uint32_t dist_extra(uint32_t d) { return d < 4u ? 0u : (d >> 1) - 1u; }
SCG_HD uint32_t dist_base(uint32_t d, uint32_t eb) { return d < 4u ? d + 1u : ((2u + (d & 1u)) << eb) + 1u; }

// The match that begins with literal/length symbol s > 256, which has just been read: the length's extra bits, the
// distance code and its extra bits.  False for a symbol or a distance code that is none.  Needs 33 bits in the reader.
template<class TablesT>
SCG_HD bool read_match(BitReader& br, const TablesT& T, int s, uint32_t& n, uint32_t& dist) {
    if (s > 285) return false;                                           // "invalid literal/length code"
    const uint32_t lt = static_cast<uint32_t>(s) - 257u, leb = length_extra(lt);
    n = length_base(lt, leb) + br.bits(leb);
    br.refill();
    const int d = decode_symbol(br, T.dtab, TablesT::dist_bits, T.dcount, T.dsym);
    if (d < 0 || d >= 30) return false;                                  // "invalid distance code"
    const uint32_t deb = dist_extra(static_cast<uint32_t>(d));
    dist = dist_base(static_cast<uint32_t>(d), deb) + br.bits(deb);
    return true;
}

// What the code starting at the low end of `w` would be (>= 57 valid bits), were it a code start.
// kind: 0 literal, 1 match, 2 end of block, 3 "not decodable here" (long code / invalid: the chain stops)
struct LaneCode {
    uint32_t kind, adv, outlen, n, dist, sym;
};
template<class TablesT>
SCG_HD LaneCode decode_here(const TablesT& T, uint64_t w) {
    // Straight-line: every lane goes through the length and the distance arithmetic, whatever its code is, and the
    // results are selected at the end.  As nested branches this cost 13 exec-mask save / restore pairs and 40 register
    // moves per 64 offsets -- scalar instructions the whole wavefront waits for, most of them for offsets that are no code
    // starts anyway.
    LaneCode c;
    const uint32_t e = T.lit[static_cast<uint32_t>(w) & ((1u << TablesT::lit_bits) - 1u)];
    const uint32_t l = e >> 12;
    c.sym = e & 0xFFFu;
    const uint32_t t0 = c.sym - 257u;                                   // (wraps for literals: clamped, and not used then)
    const uint32_t t = t0 < 28u ? t0 : 28u;
    const uint32_t eb = length_extra(t);
    const uint32_t base = length_base(t, eb);
    uint64_t w2 = w >> l;
    c.n = base + (static_cast<uint32_t>(w2) & ((1u << eb) - 1u));
    w2 >>= eb;
    const uint32_t de = T.dtab[static_cast<uint32_t>(w2) & ((1u << TablesT::dist_bits) - 1u)];
    const uint32_t dl = de >> 12, ds0 = de & 0xFFFu;
    const uint32_t ds = ds0 < 29u ? ds0 : 29u;
    const uint32_t deb = dist_extra(ds);
    const uint32_t dbase = dist_base(ds, deb);
    w2 >>= dl;
    c.dist = dbase + (static_cast<uint32_t>(w2) & ((1u << deb) - 1u));
    const bool is_length = c.sym > 256u && c.sym <= 285u;
    const bool is_match = is_length && de != 0u && ds0 < 30u;
    c.kind = e == 0u ? 3u : (c.sym < 256u ? 0u : (c.sym == 256u ? 2u : (is_match ? 1u : 3u)));
    c.adv = c.kind == 1u ? l + eb + dl + deb : l;
    c.outlen = c.kind == 0u ? 1u : (c.kind == 1u ? c.n : 0u);
    return c;
}

// The two tables of a block from its code lengths, lens[0 .. nlen) and lens[nlen .. nlen + ndist).  The distance code
// first: its lengths lie in the area the literal/length table is about to take; that table then overwrites its own
// lengths: the builder reads them before it writes.
template<class TablesT>
SCG_HD bool build_tables(TablesT& T, const uint8_t* lens, int nlen, int ndist) {
    if (!build_code(lens + nlen, ndist, 1, T.dtab, TablesT::dist_bits, T.dcount, T.dsym, T.offs)) return false;     // "invalid distances set"
    if (!build_code(lens, nlen, 1, T.lit, TablesT::lit_bits, T.lcount, T.lsym, T.offs)) return false;               // "invalid literal/lengths set"
    return true;
}

// The lengths of the fixed code (inflate.c: fixedtables): 288 literal/length codes, then 32 distance codes.
SCG_HD void fixed_code_lengths(uint8_t* lens) {
    for (int s = 0; s < 144; ++s) lens[s] = 8;
    for (int s = 144; s < 256; ++s) lens[s] = 9;
    for (int s = 256; s < 280; ++s) lens[s] = 7;
    for (int s = 280; s < 288; ++s) lens[s] = 8;
    for (int s = 0; s < 32; ++s) lens[288 + s] = 5;
}
template<class TablesT>
SCG_HD bool fixed_tables(TablesT& T, uint8_t* lens) {
    fixed_code_lengths(lens);
    return build_tables(T, lens, 288, 32);
}

// The code lengths of a dynamic-Huffman block header (br stands behind BFINAL and BTYPE, 14 bits in its buffer): nlen
// literal/length and ndist distance lengths to lens[0 ...), which has room for LENS_BYTES.  False for anything zlib would
// reject up to there (too many codes, an over-subscribed or incomplete code-length code, a repeat with nothing to repeat or
// beyond the end, no end-of-block code).  The code-length code lives in the caller's cltab (1 << CL_BITS entries), count
// (16), sym (19) and offs (16) while this runs.
template<class Reader>
SCG_HD bool read_code_lengths(Reader& br, uint8_t* lens, int& nlen, int& ndist, uint16_t* cltab, uint16_t* count, uint16_t* sym, uint16_t* offs) {
    nlen = static_cast<int>(br.bits(5)) + 257;
    ndist = static_cast<int>(br.bits(5)) + 1;
    const int ncode = static_cast<int>(br.bits(4)) + 4;
    if (nlen > 286 || ndist > 30) return false;                          // "too many length or distance symbols"
    // the code-length code: its 19 lengths sit behind the 320 bytes reserved for the lengths proper
    uint8_t* const cl = lens + 320;
    // the order of the code-length code's lengths (16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15), five bits each
    const uint64_t order_lo = 0x22caa324e804a30ull, order_hi = 0x3c2e1346cull;
    for (int i = 0; i < 19; ++i) cl[i] = 0;
    for (int i = 0; i < ncode; ++i) {
        br.refill();
        const uint32_t at = static_cast<uint32_t>((i < 12 ? order_lo >> (5 * i) : order_hi >> (5 * (i - 12))) & 31u);
        cl[at] = static_cast<uint8_t>(br.bits(3));
    }
    if (!build_code(cl, 19, 0, cltab, CL_BITS, count, sym, offs)) return false;              // "invalid code lengths set"
    int have = 0;
    while (have < nlen + ndist) {
        if (br.overrun()) return false;
        br.refill();
        const int s = decode_symbol(br, cltab, CL_BITS, count, sym);
        if (s < 0) return false;
        if (s < 16) { lens[have++] = static_cast<uint8_t>(s); continue; }
        uint8_t fill = 0;
        int rep;
        if (s == 16) {
            if (have == 0) return false;                                 // "invalid bit length repeat"
            fill = lens[have - 1];
            rep = 3 + static_cast<int>(br.bits(2));
        } else if (s == 17) {
            rep = 3 + static_cast<int>(br.bits(3));
        } else {
            rep = 11 + static_cast<int>(br.bits(7));
        }
        if (have + rep > nlen + ndist) return false;                     // "invalid bit length repeat"
        while (rep--) lens[have++] = fill;
    }
    return lens[256] != 0;                                               // "invalid code -- missing end-of-block"
}

// A dynamic-Huffman block header and the block's two tables; false for anything zlib would reject.
// (the code-length code borrows the distance code's arrays, which are built afterwards)
template<class TablesT>
SCG_HD bool read_dynamic_tables(BitReader& br, TablesT& T, uint8_t* lens) {
    int nlen, ndist;
    if (!read_code_lengths(br, lens, nlen, ndist, T.dtab, T.dcount, T.dsym, T.offs)) return false;
    return build_tables(T, lens, nlen, ndist);
}

// The dynamic block filter -- the cheap test that proposes block starts to the chunked gzip decoders (BFINAL = 0, BTYPE = 2,
// HLIT and HDIST <= 29, Kraft sum of the code-length code = 128) -- is the ONE rule that stays spelled twice: branch-free
// in gunzip_find_kernel (scg_inflate.hip), with early exits in pgz::find_dynamic_block (scg_pgzip.h).  As one branch-free
// function here it was tried and measured slower on both sides (profiles/gzip_rules_ab.txt).  It only proposes: what passes
// is parsed in full by read_code_lengths, so a drift between the two moves where chunks start, never what is accepted.

// The decoder writes bytes (BGZF members: the text itself) or 16-bit symbols (chunks of an ordinary gzip stream, decoded
// without the 32 KiB of text in front of them: a symbol is a byte, or MARKER + k for "byte k of the window I do not have";
// scg_pgzip.h).  In symbol mode a match may reach in front of the chunk's first symbol: those positions read as markers.
constexpr uint32_t MARKER = 0x8000u, MARKER_WINDOW = 32768u;

// What stands `-from` symbols in front of the chunk (from < 0).
SCG_HD uint16_t marker_before(int32_t from) { return static_cast<uint16_t>(MARKER + MARKER_WINDOW + from); }

// One match, copied by one lane: out[at + j] = out[at - d + j], j < len, in that order (d < len: a pattern of period d).
// E is a byte or a 16-bit symbol, W of them to a word.  A source at least a word back is moved in 8-byte words (up to
// four loads in flight); a closer one is a pattern of period d, built once in a register and stored over and over.
// Writes nothing beyond at + len.  READS whole words: for d < W the W elements from at - d on, so up to W - 1 elements
// at and behind `at` that are not text yet (never used), of which W - d - len (4 bytes at the most, no symbols) may lie
// beyond at + len: the buffer owns that slack.  In bytes d <= at is the caller's business; in symbols a match that
// begins in front of the chunk goes symbol by symbol.
template<class E>
SCG_HD void copy_match(E* out, uint32_t at, uint32_t len, uint32_t d) {
    constexpr uint32_t W = 8 / sizeof(E), BITS = 8 * sizeof(E);
    E* dst = out + at;
    if (sizeof(E) == 2 && at < d) {
        for (uint32_t j = 0; j < len; ++j) {
            const int32_t from = static_cast<int32_t>(at + j) - static_cast<int32_t>(d);
            dst[j] = from < 0 ? static_cast<E>(marker_before(from)) : out[from];
        }
        return;
    }
    const E* src = dst - d;
    uint32_t j = 0;
    uint64_t w;
    if (d >= W) {
        if (d >= 4 * W) {
            for (; j + 4 * W <= len; j += 4 * W) {
                uint64_t x[4];
                for (uint32_t k = 0; k < 4; ++k) __builtin_memcpy(&x[k], src + j + W * k, 8);
                for (uint32_t k = 0; k < 4; ++k) __builtin_memcpy(dst + j + W * k, &x[k], 8);
            }
        }
        for (; j + W <= len; j += W) {
            __builtin_memcpy(&w, src + j, 8);
            __builtin_memcpy(dst + j, &w, 8);
        }
        if (j < len) __builtin_memcpy(&w, src + j, 8);          // (ends at most where this match's own text begins)
    } else {
        __builtin_memcpy(&w, src, 8);                           // the d elements of the pattern and W - d that are not text yet
        w &= ~0ull >> (64u - BITS * d);
        for (uint32_t have = d; have < W; have <<= 1) w |= w << (BITS * have);
        // the largest multiple of d within a word, (W / d) * d, spelled out: a division costs the device twenty instructions
        const uint32_t step = W == 8 ? (d == 3 ? 6u : (d >= 5 ? d : 8u)) : (d == 3 ? 3u : 4u);
        for (; j + W <= len; j += step) __builtin_memcpy(dst + j, &w, 8);
    }
    for (uint32_t k = 0; j + k < len; ++k) dst[j + k] = static_cast<E>(w >> (BITS * k));
}

// Inflates the raw DEFLATE stream in[0 .. in_len) into out[0 .. out_len): INFLATE_OK only if the stream is valid, ends
// exactly at in_len and produces exactly out_len bytes.  in must be readable up to in_len + IN_SLACK.
template<class Wave>
SCG_HD int inflate_member(const uint8_t* in, uint32_t in_len, uint8_t* out, uint32_t out_len, LaneTables& T, const Wave& wave) {
    BitReader br;
    br.open(in, in_len);
    TextWriter<Wave> w(wave, out);
    uint32_t& op = w.op;
    uint8_t* const lens = reinterpret_cast<uint8_t*>(T.lit);             // 320 code lengths fit the 1 KiB of T.lit
    uint32_t last;
    do {
        if (br.overrun()) return INFLATE_BAD_DATA;
        br.refill();
        last = br.bits(1);
        const uint32_t type = br.bits(2);
        if (type == 0) {
            // stored block: LEN, ~LEN at the next byte boundary, then LEN bytes
            br.bits(br.cnt & 7u);
            br.refill();
            br.refill();
            const uint32_t n = br.bits(16), nn = br.bits(16);
            if ((n ^ 0xFFFFu) != nn) return INFLATE_BAD_DATA;           // "invalid stored block lengths"
            if (n > out_len - op) return INFLATE_BAD_SIZE;
            uint32_t left = n;
            while (left && br.cnt) {
                w.literal(br.bits(8));
                --left;
            }
            if (left) {
                // the bit buffer is empty: br.pos is the next byte of the stream
                if (br.pos > in_len || left > in_len - br.pos) return INFLATE_BAD_DATA;
                w.raw(in + br.pos, left);
                br.seek(br.pos + left);
            }
            continue;
        }
        if (type == 3) return INFLATE_BAD_DATA;                          // "invalid block type"
        if (type == 1) {
            if (!fixed_tables(T, lens)) return INFLATE_BAD_DATA;
        } else if (!read_dynamic_tables(br, T, lens)) {
            return INFLATE_BAD_DATA;
        }
        for (;;) {
            if (br.overrun()) return INFLATE_BAD_DATA;
            br.refill();
            const int s = decode_symbol(br, T.lit, LIT_BITS, T.lcount, T.lsym);
            if (s < 0) return INFLATE_BAD_DATA;                          // "invalid literal/length code"
            if (s < 256) {
                if (op >= out_len) return INFLATE_BAD_SIZE;
                w.literal(static_cast<uint32_t>(s));
                continue;
            }
            if (s == 256) break;
            uint32_t n, dist;
            if (!read_match(br, T, s, n, dist)) return INFLATE_BAD_DATA;
            if (dist > op) return INFLATE_BAD_DATA;                      // "invalid distance too far back"
            if (n > out_len - op) return INFLATE_BAD_SIZE;
            w.match(n, dist);
        }
    } while (!last);
    w.finish();
    // the stream must end where the member's payload ends, and fill the announced size
    const uint32_t consumed = br.pos - (br.cnt >> 3);
    if (consumed != in_len || op != out_len) return INFLATE_BAD_SIZE;
    return INFLATE_OK;
}

// ---- CRC-32 of a text from the CRCs of its pieces ----
// crc(A B) = crc(A) * x^(8 |B|) + crc(B) over GF(2) modulo the CRC polynomial (zlib's crc32_combine).
// a * b mod p, reflected: bit 31 is x^0 (crc32.c: multmodp).
SCG_HD uint32_t gf2_mult(uint32_t a, uint32_t b) {
    uint32_t p = 0;
    for (int i = 0; i < 32 && a; ++i) {        // bit 31 of a first; done when no bits of a are left
        if (a & 0x80000000u) p ^= b;
        a <<= 1;
        b = (b & 1u) ? (b >> 1) ^ 0xEDB88320u : b >> 1;
    }
    return p;
}
// x^(8 len): the factor that moves a CRC across len bytes.  By squaring (x^1, x^2, x^4 ...: the series the device's table
// of powers holds, scg_inflate.hip: crc_powers) -- zlib's crc32_combine in its 1.2.11 form squares a 32 x 32 matrix per
// call; thousands of pieces of one length need the power only once.
constexpr uint32_t GF2_X0 = 0x80000000u, GF2_X1 = 0x40000000u;
SCG_HD uint32_t x_pow_bytes(uint64_t len) {
    uint32_t sq = GF2_X1, x = GF2_X0;
    for (int k = 0; k < 3; ++k) sq = gf2_mult(sq, sq);          // x^8
    for (; len; len >>= 1) {
        if (len & 1u) x = gf2_mult(sq, x);
        sq = gf2_mult(sq, sq);
    }
    return x;
}

}  // namespace scginf

#endif
