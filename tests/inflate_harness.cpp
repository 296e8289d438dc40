// inflate_harness.cpp -- host-side differential test of csrc/scg_inflate.h (the DEFLATE rules of the device inflate
// kernels) against zlib: the per-wavefront decoder as it is, and a model of the lane-parallel decoder built from the
// functions that decoder shares with it.  Built by tests/test_inflate_cpu.py with g++ -fsanitize=address,undefined.
//   inflate_harness <seed> <rounds>
//   inflate_harness --streams FILE
// Valid streams of many shapes (levels 0-9, Z_FIXED / Z_HUFFMAN_ONLY / Z_RLE / Z_FILTERED, FASTQ-like, random, runs)
// must decode identically; corrupted streams must be rejected whenever zlib rejects them and, when accepted, give
// exactly zlib's output; nothing may read or write out of bounds (ASan) or run away.
// --streams: FILE holds hand-written streams (tests/test_deflate_shapes_cpu.py), entry after entry: u32 stream bytes, u32 text
// bytes, u8 valid, the stream, the text (little endian).  Each runs through ours(): accept / reject must equal zlib's verdict
// and the entry's flag, and accepted text must equal the entry's.
#include "../screencounter_amd/csrc/scg_inflate.h"
#include "../screencounter_amd/csrc/scg_pgzip.h"

#include <zlib.h>

#include <algorithm>
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <random>
#include <string>
#include <vector>

static std::vector<uint8_t> make_data(std::mt19937_64& rng, int kind, size_t n) {
    std::vector<uint8_t> d(n);
    switch (kind) {
        case 0: {   // FASTQ-like
            size_t i = 0;
            uint64_t id = rng();
            while (i < n) {
                char name[96];
                int m = snprintf(name, sizeof(name), "@INSTR:%llu:FLOW:1:%llu:%llu 1:N:0:ACGT\n", (unsigned long long)(id % 97), (unsigned long long)(id % 100000), (unsigned long long)(rng() % 100000));
                ++id;
                for (int k = 0; k < m && i < n; ++k) d[i++] = (uint8_t)name[k];
                const int L = 20 + (int)(rng() % 140);
                for (int k = 0; k < L && i < n; ++k) d[i++] = (uint8_t)"ACGTN"[(rng() % 100) < 99 ? rng() % 4 : 4];
                if (i < n) d[i++] = '\n';
                if (i < n) d[i++] = '+';
                if (i < n) d[i++] = '\n';
                for (int k = 0; k < L && i < n; ++k) d[i++] = (uint8_t)("FFFF:FF,F#"[rng() % 10]);
                if (i < n) d[i++] = '\n';
            }
            break;
        }
        case 1: for (auto& b : d) b = (uint8_t)rng(); break;                            // incompressible
        case 2: for (auto& b : d) b = 0; break;                                          // one long run
        case 3: for (size_t i = 0; i < n; ++i) d[i] = (uint8_t)("abcabcabd"[i % 9]); break;  // short periods: overlapping copies
        case 4: for (auto& b : d) b = (uint8_t)(rng() % 3 ? 'a' + rng() % 4 : rng()); break; // skewed alphabet: long and short codes
        case 5: {   // many distinct symbols with geometric frequencies: code lengths up to 15
            for (auto& b : d) { int k = 0; while (k < 200 && (rng() & 1)) ++k; b = (uint8_t)k; }
            break;
        }
        default: for (size_t i = 0; i < n; ++i) d[i] = (uint8_t)(i * 7 + (i >> 8)); break;
    }
    return d;
}

static std::vector<uint8_t> deflate_raw(const std::vector<uint8_t>& d, int level, int strategy, int flush_every) {
    z_stream zs;
    memset(&zs, 0, sizeof(zs));
    if (deflateInit2(&zs, level, Z_DEFLATED, -15, 8, strategy) != Z_OK) abort();
    std::vector<uint8_t> out(deflateBound(&zs, d.size()) + 64 + (flush_every ? d.size() / flush_every * 16 : 0));
    zs.next_out = out.data();
    zs.avail_out = (uInt)out.size();
    size_t at = 0;
    while (flush_every && at + flush_every < d.size()) {      // several blocks, incl. empty stored ones from Z_FULL_FLUSH
        zs.next_in = const_cast<Bytef*>(d.data() + at);
        zs.avail_in = (uInt)flush_every;
        if (deflate(&zs, (at / flush_every) % 2 ? Z_FULL_FLUSH : Z_SYNC_FLUSH) != Z_OK) abort();
        at += flush_every;
    }
    zs.next_in = const_cast<Bytef*>(d.data() + at);
    zs.avail_in = (uInt)(d.size() - at);
    if (deflate(&zs, Z_FINISH) != Z_STREAM_END) abort();
    out.resize(zs.total_out);
    deflateEnd(&zs);
    return out;
}

// zlib's verdict on a raw stream that must produce exactly n bytes from exactly the whole input.
static bool zlib_inflate(const std::vector<uint8_t>& c, size_t n, std::vector<uint8_t>& out) {
    z_stream zs;
    memset(&zs, 0, sizeof(zs));
    if (inflateInit2(&zs, -15) != Z_OK) abort();
    out.assign(n + 1, 0);
    zs.next_in = const_cast<Bytef*>(c.data());
    zs.avail_in = (uInt)c.size();
    zs.next_out = out.data();
    zs.avail_out = (uInt)out.size();
    const int rc = inflate(&zs, Z_FINISH);
    const bool ok = rc == Z_STREAM_END && zs.total_out == n && zs.avail_in == 0;
    inflateEnd(&zs);
    out.resize(n);
    return ok;
}

// The lane-parallel decoder's arithmetic without its scheduling (scg_inflate.hip: inflate_lanes / inflate_member_lanes):
// the same tables, and at every code start decode_here on the 64 bits found there -- the device does that for 128 bit
// offsets at once and then walks the chain of true code starts; here the chain is walked one start at a time, and a
// match is copied at once (copy_match) where the device defers it.  What decode_here does not resolve (kind 3) takes
// the bitwise path, as on the device.  OutT = uint8_t: a BGZF member's text; uint16_t: symbols, with nothing in front.
constexpr size_t COPY_SLACK = 8;        // bytes behind the output that copy_match may read (scg_inflate.h)
template<class OutT>
static int lanes_model(const uint8_t* in, uint32_t in_len, OutT* out, uint32_t out_len) {
    using namespace scginf;
    static WaveTables T;
    uint32_t bitpos = 0, op = 0, last;
    const uint32_t in_bits = in_len * 8u;
    do {
        if (bitpos > in_bits) return INFLATE_BAD_DATA;
        BitReader br;
        br.open_at_bit(in, in_len, bitpos);
        last = br.bits(1);
        const uint32_t type = br.bits(2);
        if (type == 0) {
            br.bits(br.cnt & 7u);
            br.refill();
            br.refill();
            const uint32_t n = br.bits(16), nn = br.bits(16);
            if ((n ^ 0xFFFFu) != nn) return INFLATE_BAD_DATA;
            if (n > out_len - op) return INFLATE_BAD_SIZE;
            const uint32_t from = br.pos - (br.cnt >> 3);
            if (from > in_len || n > in_len - from) return INFLATE_BAD_DATA;
            for (uint32_t j = 0; j < n; ++j) out[op + j] = in[from + j];
            op += n;
            bitpos = (from + n) * 8u;
            continue;
        }
        if (type == 3) return INFLATE_BAD_DATA;
        uint8_t* const lens = reinterpret_cast<uint8_t*>(T.lit);
        if (!(type == 1 ? fixed_tables(T, lens) : read_dynamic_tables(br, T, lens))) return INFLATE_BAD_DATA;
        bitpos = br.bit_position();
        for (bool block_done = false; !block_done;) {
            if (bitpos > in_bits) return INFLATE_BAD_DATA;
            uint64_t w;                                                  // (the device's ring reads zeros beyond in_len + IN_SLACK)
            memcpy(&w, in + (bitpos >> 3), 8);
            const LaneCode c = decode_here(T, w >> (bitpos & 7u));
            if (c.kind == 0) {
                if (op >= out_len) return INFLATE_BAD_SIZE;
                out[op++] = static_cast<OutT>(c.sym);
                bitpos += c.adv;
            } else if (c.kind == 1) {
                if (sizeof(OutT) == 1 && c.dist > op) return INFLATE_BAD_DATA;
                if (c.n > out_len - op) return INFLATE_BAD_SIZE;
                copy_match(out, op, c.n, c.dist);
                op += c.n;
                bitpos += c.adv;
            } else if (c.kind == 2) {
                bitpos += c.adv;
                block_done = true;
            } else {
                BitReader sr;
                sr.open_at_bit(in, in_len, bitpos);
                const int s = decode_symbol(sr, T.lit, LANES_LIT_BITS, T.lcount, T.lsym);
                if (s < 0) return INFLATE_BAD_DATA;
                if (s < 256) {
                    if (op >= out_len) return INFLATE_BAD_SIZE;
                    out[op++] = static_cast<OutT>(s);
                } else if (s == 256) {
                    block_done = true;
                } else {
                    uint32_t len, d;
                    if (!read_match(sr, T, s, len, d)) return INFLATE_BAD_DATA;
                    if (sizeof(OutT) == 1 && d > op) return INFLATE_BAD_DATA;
                    if (len > out_len - op) return INFLATE_BAD_SIZE;
                    copy_match(out, op, len, d);
                    op += len;
                }
                bitpos = sr.bit_position();
            }
        }
    } while (!last);
    if (((bitpos + 7u) >> 3) != in_len || op != out_len) return INFLATE_BAD_SIZE;
    return INFLATE_OK;
}

// The host's chunk decoder (scg_pgzip.h: its own tables and loop over the same rules), block after block from the member's
// first bit with nothing in front (reach 0).  Accepted only if the last block is final, the stream ends in the input's
// last byte and the text has exactly n symbols.  out: n + 16 symbols (the slack pgz::copy_match announces); in: size +
// pgz::IN_SLACK bytes.
static bool host_chunk_decoder(const uint8_t* in, size_t size, uint16_t* out, size_t n) {
    using namespace scg::pgz;
    static Tables T;
    uint8_t lens[scginf::LENS_BYTES];
    Bits br;
    uint64_t bit = 0;
    size_t op = 0;
    int rc;
    do {
        br.open(in, size, bit);
        rc = decode_block(br, T, out, op, n, 0, lens);
        bit = br.bitpos();
    } while (rc == BLOCK_OK);
    return rc == BLOCK_FINAL && ((bit + 7) >> 3) == size && op == n;
}

// The decoder with "wavefronts" of 1, 7 and 64 lanes (the device runs 64): all must agree, byte for byte and verdict
// for verdict -- the wider ones exercise the batched literals and the deferred stores of short matches.  So must the model
// of the lane-parallel decoder, in bytes and -- whatever is accepted -- in symbols, where no marker may appear: nothing
// reaches in front of a member's start.  And so must the host's chunk decoder, which takes what the device hands back.
static int ours(const std::vector<uint8_t>& c, size_t n, std::vector<uint8_t>& out) {
    // exact-size buffers so that ASan sees any access beyond the slack or the output
    std::vector<uint8_t> in(c.size() + scginf::IN_SLACK, 0xA5);
    memcpy(in.data(), c.data(), c.size());
    static scginf::LaneTables T;
    out.assign(n, 0xEE);
    const int rc = scginf::inflate_member(in.data(), (uint32_t)c.size(), out.data(), (uint32_t)n, T, scginf::HostWave<64>());
    std::vector<uint8_t> o1(n, 0xEE), o7(n, 0xEE);
    const int rc1 = scginf::inflate_member(in.data(), (uint32_t)c.size(), o1.data(), (uint32_t)n, T, scginf::HostWave<1>());
    const int rc7 = scginf::inflate_member(in.data(), (uint32_t)c.size(), o7.data(), (uint32_t)n, T, scginf::HostWave<7>());
    // (which of the two error codes a broken stream earns may depend on where a run of literals is cut: both mean "not this decoder's")
    const bool ok = rc == scginf::INFLATE_OK;
    if ((rc1 == scginf::INFLATE_OK) != ok || (rc7 == scginf::INFLATE_OK) != ok || (ok && (o1 != out || o7 != out))) {
        fprintf(stderr, "FAIL the lane widths disagree: rc %d / %d / %d\n", rc, rc1, rc7);
        exit(1);
    }
    // exact-size buffers again, but for the slack that copy_match announces
    std::vector<uint8_t> ob(n + COPY_SLACK, 0xEE);
    const int rcb = lanes_model(in.data(), (uint32_t)c.size(), ob.data(), (uint32_t)n);
    if ((rcb == scginf::INFLATE_OK) != ok || (ok && !std::equal(out.begin(), out.end(), ob.begin()))) {
        fprintf(stderr, "FAIL the lane-parallel model disagrees: rc %d where the wavefront decoder says %d\n", rcb, rc);
        exit(1);
    }
    if (ok) {
        std::vector<uint16_t> os(n + COPY_SLACK / 2, 0xEEEE);
        const int rcs = lanes_model(in.data(), (uint32_t)c.size(), os.data(), (uint32_t)n);
        bool same = rcs == scginf::INFLATE_OK;
        for (size_t i = 0; same && i < n; ++i) same = os[i] == out[i];             // (a marker is >= 0x8000: no byte)
        if (!same) {
            fprintf(stderr, "FAIL the lane-parallel model in symbols: rc %d, or symbols that are not the text\n", rcs);
            exit(1);
        }
    }
    {
        std::vector<uint8_t> hin(c.size() + scg::pgz::IN_SLACK, 0xA5);
        memcpy(hin.data(), c.data(), c.size());
        std::vector<uint16_t> hs(n + 16, 0xEEEE);
        bool same = host_chunk_decoder(hin.data(), c.size(), hs.data(), n) == ok;
        for (size_t i = 0; ok && same && i < n; ++i) same = hs[i] == out[i];        // (no symbol above 255: no marker)
        if (!same) {
            fprintf(stderr, "FAIL the host chunk decoder disagrees with the wavefront decoder's rc %d, or its symbols are not the text\n", rc);
            exit(1);
        }
    }
    return rc;
}

static int run_streams(const char* path) {
    FILE* f = fopen(path, "rb");
    if (!f) { fprintf(stderr, "FAIL cannot open %s\n", path); return 1; }
    long entries = 0, valid = 0;
    for (;;) {
        uint8_t head[9];
        const size_t got_head = fread(head, 1, sizeof(head), f);
        if (got_head == 0) break;
        if (got_head != sizeof(head)) { fprintf(stderr, "FAIL truncated container (entry %ld)\n", entries); return 1; }
        uint32_t clen, tlen;
        memcpy(&clen, head, 4);
        memcpy(&tlen, head + 4, 4);
        const bool want = head[8] != 0;
        std::vector<uint8_t> c(clen), text(tlen);
        if ((clen && fread(c.data(), 1, clen, f) != clen) || (tlen && fread(text.data(), 1, tlen, f) != tlen)) {
            fprintf(stderr, "FAIL truncated container (entry %ld)\n", entries);
            return 1;
        }
        std::vector<uint8_t> zout, mine;
        const bool zok = zlib_inflate(c, tlen, zout);
        const int rc = ours(c, tlen, mine);
        const bool ok = rc == scginf::INFLATE_OK;
        if (zok != want) { fprintf(stderr, "FAIL entry %ld: zlib %s a stream marked %s\n", entries, zok ? "accepts" : "rejects", want ? "valid" : "invalid"); return 1; }
        if (ok != zok) { fprintf(stderr, "FAIL entry %ld: rc %d where zlib %s\n", entries, rc, zok ? "accepts" : "rejects"); return 1; }
        if (ok && (mine != text || zout != text)) { fprintf(stderr, "FAIL entry %ld: the text differs from the intended one\n", entries); return 1; }
        ++entries;
        valid += want;
    }
    fclose(f);
    printf("ok: %ld streams (%ld valid, %ld invalid)\n", entries, valid, entries - valid);
    return 0;
}

int main(int argc, char** argv) {
    if (argc > 2 && strcmp(argv[1], "--streams") == 0) return run_streams(argv[2]);
    const uint64_t seed = argc > 1 ? strtoull(argv[1], nullptr, 10) : 1;
    const int rounds = argc > 2 ? atoi(argv[2]) : 200;
    std::mt19937_64 rng(seed);
    long valid = 0, corrupt = 0, corrupt_accepted = 0, size_variants = 0;
    const int strategies[5] = {Z_DEFAULT_STRATEGY, Z_FIXED, Z_HUFFMAN_ONLY, Z_RLE, Z_FILTERED};
    for (int r = 0; r < rounds; ++r) {
        const int kind = (int)(rng() % 7);
        const size_t n = (r % 11 == 0) ? rng() % 40 : (r % 7 == 0 ? 65280 : 1 + rng() % 70000);
        const std::vector<uint8_t> d = make_data(rng, kind, n);
        const int level = (int)(rng() % 10);
        const int strategy = strategies[rng() % 5];
        const int flush_every = (rng() % 3 == 0 && n > 64) ? (int)(16 + rng() % (n / 2)) : 0;
        const std::vector<uint8_t> c = deflate_raw(d, level, strategy, flush_every);
        std::vector<uint8_t> got;
        const int rc = ours(c, n, got);
        if (rc != scginf::INFLATE_OK || got != d) {
            fprintf(stderr, "FAIL valid stream: round %d kind %d n %zu level %d strategy %d flush %d rc %d\n", r, kind, n, level, strategy, flush_every, rc);
            return 1;
        }
        ++valid;
        // wrong announced sizes must be rejected
        if (n > 0) {
            if (ours(c, n - 1, got) == scginf::INFLATE_OK) { fprintf(stderr, "FAIL short output accepted (round %d)\n", r); return 1; }
        }
        if (ours(c, n + 1, got) == scginf::INFLATE_OK) { fprintf(stderr, "FAIL long output accepted (round %d)\n", r); return 1; }
        {
            std::vector<uint8_t> c2 = c;
            c2.push_back(0);
            if (ours(c2, n, got) == scginf::INFLATE_OK) { fprintf(stderr, "FAIL trailing input accepted (round %d)\n", r); return 1; }
            if (c.size() > 1) {
                c2.assign(c.begin(), c.end() - 1);
                std::vector<uint8_t> z;
                if (ours(c2, n, got) == scginf::INFLATE_OK && !zlib_inflate(c2, n, z)) { fprintf(stderr, "FAIL truncated input accepted (round %d)\n", r); return 1; }
            }
            size_variants += 4;
        }
        // corrupted streams: bit flips, byte smashes, early in the header and anywhere
        for (int k = 0; k < 12 && !c.empty(); ++k) {
            std::vector<uint8_t> bad = c;
            const int flips = 1 + (int)(rng() % 3);
            for (int f = 0; f < flips; ++f) {
                const size_t where = (k % 3 == 0) ? rng() % std::min<size_t>(bad.size(), 24) : rng() % bad.size();
                if (rng() % 4 == 0) bad[where] = (uint8_t)rng(); else bad[where] ^= (uint8_t)(1u << (rng() % 8));
            }
            std::vector<uint8_t> zout, mine;
            const bool zok = zlib_inflate(bad, n, zout);
            const int mrc = ours(bad, n, mine);
            ++corrupt;
            if (mrc == scginf::INFLATE_OK) {
                ++corrupt_accepted;
                if (!zok) { fprintf(stderr, "FAIL accepted a stream zlib rejects: round %d variant %d\n", r, k); return 1; }
                if (mine != zout) { fprintf(stderr, "FAIL output differs from zlib on an accepted corrupted stream: round %d variant %d\n", r, k); return 1; }
            }
            // (rejecting a stream zlib accepts only costs a fall-back to the host path, but it should not happen either)
            if (zok && mrc != scginf::INFLATE_OK) { fprintf(stderr, "FAIL rejected a stream zlib accepts: round %d variant %d rc %d\n", r, k, mrc); return 1; }
        }
    }
    printf("ok: %ld valid streams, %ld size variants, %ld corrupted streams (%ld still valid and identical to zlib)\n", valid, size_variants, corrupt, corrupt_accepted);
    return 0;
}
