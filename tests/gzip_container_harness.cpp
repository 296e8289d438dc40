// gzip_container_harness.cpp -- the gzip container parsers of csrc/scg_gzip.h (member header, BGZF size subfield,
// trailer) on headers built by hand.  Every buffer is a heap block of exactly the bytes the parser is told about, so
// that AddressSanitizer sees a single byte read beyond them.  Built and run by tests/test_gzip_container_cpu.py, plain
// and with -fsanitize=address,undefined.  Prints "ok: <checks>" or "FAIL ...".
#include "../screencounter_amd/csrc/scg_gzip.h"

#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <string>
#include <vector>

using namespace scg::gz;
typedef std::vector<uint8_t> Bytes;

static long checks = 0;
#define CHECK(cond, ...)                                                                  \
    do {                                                                                  \
        ++checks;                                                                         \
        if (!(cond)) { std::printf("FAIL line %d: %s: ", __LINE__, #cond); std::printf(__VA_ARGS__); std::printf("\n"); std::exit(1); } \
    } while (0)

// The first n bytes of b in a block of exactly n bytes.
static std::unique_ptr<uint8_t[]> exact(const Bytes& b, size_t n) {
    std::unique_ptr<uint8_t[]> p(new uint8_t[n ? n : 1]);
    if (n) std::memcpy(p.get(), b.data(), n);
    return p;
}

static void put16(Bytes& b, size_t v) { b.push_back(uint8_t(v)); b.push_back(uint8_t(v >> 8)); }

// A member header: the ten fixed bytes, then what the flags announce.
static Bytes header(uint8_t flags, const Bytes& extra = {}, const std::string& name = "", const std::string& comment = "") {
    Bytes b = {0x1f, 0x8b, 8, flags, 1, 2, 3, 4, 0, 3};      // (MTIME 1 2 3 4, XFL 0, OS 3)
    if (flags & FEXTRA) { put16(b, extra.size()); b.insert(b.end(), extra.begin(), extra.end()); }
    if (flags & FNAME) { b.insert(b.end(), name.begin(), name.end()); b.push_back(0); }
    if (flags & FCOMMENT) { b.insert(b.end(), comment.begin(), comment.end()); b.push_back(0); }
    if (flags & FHCRC) put16(b, 0xBEEF);
    return b;
}

static Bytes subfield(char a, char b, const Bytes& data) {
    Bytes s = {uint8_t(a), uint8_t(b)};
    put16(s, data.size());
    s.insert(s.end(), data.begin(), data.end());
    return s;
}
static Bytes operator+(Bytes a, const Bytes& b) { a.insert(a.end(), b.begin(), b.end()); return a; }

// The header h (at offset `front` behind bytes that are none) parses in a buffer that ends with it -- and with `behind`
// bytes more -- to the expected fields; a buffer that ends at any byte before the header's end gives false.
static MemberHeader whole_and_cut(const char* what, const Bytes& h, size_t want_extra_len, size_t front = 0) {
    Bytes b(front, 0x1f);
    b.insert(b.end(), h.begin(), h.end());
    MemberHeader got{};
    for (size_t behind : {size_t(0), size_t(1), size_t(40)}) {
        Bytes c = b;
        c.resize(b.size() + behind, 0);
        const auto p = exact(c, c.size());
        MemberHeader m{0xFF, 99, 99, 99};
        CHECK(parse_member_header(p.get(), c.size(), front, m), "%s, %zu bytes behind", what, behind);
        CHECK(m.flags == h[3] && m.payload == b.size(), "%s: flags %u payload %zu, header ends at %zu", what, m.flags, m.payload, b.size());
        CHECK(m.extra_len == want_extra_len && (m.extra_at == ((h[3] & FEXTRA) ? front + 12 : 0)), "%s: extra field %zu + %zu", what, m.extra_at, m.extra_len);
        got = m;
    }
    for (size_t n = 0; n < b.size(); ++n) {
        const auto p = exact(b, n);
        MemberHeader m{};
        CHECK(!parse_member_header(p.get(), n, front, m), "%s: accepted with %zu of %zu bytes", what, n, b.size());
    }
    return got;
}

static size_t block_size_of(const Bytes& extra) {
    const Bytes h = header(FEXTRA, extra);
    const auto p = exact(h, h.size());                      // (the buffer ends with the extra field)
    MemberHeader m{};
    CHECK(parse_member_header(p.get(), h.size(), 0, m), "extra field of %zu bytes", extra.size());
    return bgzf_block_size(p.get(), m);
}

int main() {
    const Bytes some = subfield('X', 'Y', {1, 2, 3});
    // each field alone, and all together
    whole_and_cut("no fields", header(0), 0);
    whole_and_cut("FEXTRA", header(FEXTRA, some), some.size());
    whole_and_cut("FNAME", header(FNAME, {}, "reads.fastq"), 0);
    whole_and_cut("FCOMMENT", header(FCOMMENT, {}, "", "a comment"), 0);
    whole_and_cut("FHCRC", header(FHCRC), 0);
    whole_and_cut("all fields", header(FEXTRA | FNAME | FCOMMENT | FHCRC, some, "reads.fastq", "a comment"), some.size());
    whole_and_cut("all fields, empty strings", header(FEXTRA | FNAME | FCOMMENT | FHCRC, {}, "", ""), 0);
    whole_and_cut("all fields, not at the buffer's start", header(FEXTRA | FNAME | FCOMMENT | FHCRC, some, "n", "c"), some.size(), 37);
    // XLEN = 0 and XLEN = 65535
    whole_and_cut("XLEN 0", header(FEXTRA), 0);
    whole_and_cut("XLEN 0, a name behind", header(FEXTRA | FNAME, {}, "x"), 0);
    whole_and_cut("XLEN 65535", header(FEXTRA | FNAME, Bytes(65535, 'e'), "x"), 65535);
    CHECK(block_size_of({}) == 0, "XLEN 0 holds no BC subfield");
    CHECK(block_size_of(Bytes(65535, 0)) == 0, "65535 zero bytes hold no BC subfield");       // (subfields of SLEN 0 all the way; 3 bytes left over)
    // reserved flag bits are reported, not judged
    for (uint8_t flags : {uint8_t(0x20), uint8_t(0x40), uint8_t(0x80), uint8_t(0xE0 | FNAME)}) {
        const MemberHeader m = whole_and_cut("reserved flags", header(flags, {}, "n"), 0);
        CHECK(m.flags == flags, "flags %u", m.flags);
    }
    // what is no header
    {
        Bytes h = header(0);
        for (int k = 0; k < 3; ++k) {
            Bytes bad = h + Bytes(8, 0);
            bad[k] ^= 1;                                        // magic, magic, CM
            MemberHeader m{};
            CHECK(!parse_member_header(exact(bad, bad.size()).get(), bad.size(), 0, m), "byte %d", k);
        }
        MemberHeader m{};
        const auto p = exact(h, h.size());
        CHECK(!parse_member_header(p.get(), h.size(), h.size(), m), "off == size");
        CHECK(!parse_member_header(p.get(), h.size(), h.size() + 5, m), "off > size");
        CHECK(!parse_member_header(p.get(), h.size(), 1, m), "off + 10 > size");
    }
    // an unterminated name or comment running to the buffer's end
    {
        Bytes h = header(FNAME, {}, "name_without_its_end");
        h.pop_back();
        MemberHeader m{};
        CHECK(!parse_member_header(exact(h, h.size()).get(), h.size(), 0, m), "unterminated name");
        h = header(FNAME | FCOMMENT, {}, "name", "comment_without_its_end");
        h.pop_back();
        CHECK(!parse_member_header(exact(h, h.size()).get(), h.size(), 0, m), "unterminated comment");
        // ... is nothing to a caller that walks the extra field only (BGZF): the payload then counts from behind that field
        h = header(FEXTRA | FNAME | FHCRC, some, "name_without_its_end");
        h.resize(12 + some.size() + 4);
        CHECK(parse_member_header(exact(h, h.size()).get(), h.size(), 0, m, FEXTRA) && m.payload == 12 + some.size() && m.flags == (FEXTRA | FNAME | FHCRC),
              "walk FEXTRA only: payload %zu", m.payload);
        CHECK(!parse_member_header(exact(h, 12 + some.size() - 1).get(), 12 + some.size() - 1, 0, m, FEXTRA), "walk FEXTRA only, cut in the field");
    }
    // the BC subfield: BSIZE = the member's size - 1
    const Bytes bc = subfield('B', 'C', {0x34, 0x12});
    CHECK(block_size_of(bc) == 0x1235, "BC alone (what bgzip writes)");
    CHECK(block_size_of(bc + some) == 0x1235, "BC first");
    CHECK(block_size_of(some + bc) == 0x1235, "BC behind another subfield");
    CHECK(block_size_of(some + subfield('B', 'X', {9, 9}) + subfield('X', 'C', {}) + bc) == 0x1235, "BC last");
    CHECK(block_size_of(subfield('B', 'C', {0xFF, 0xFF})) == 65536, "the largest BSIZE");
    CHECK(block_size_of(subfield('B', 'C', {1, 2, 3})) == 0, "SLEN 3");
    CHECK(block_size_of(subfield('B', 'C', {1})) == 0, "SLEN 1");
    CHECK(block_size_of(subfield('B', 'C', {1, 2, 3}) + bc) == 0x1235, "a BC of SLEN 3 in front of the real one");
    CHECK(block_size_of(some + some) == 0, "no BC");
    for (size_t keep = 0; keep < bc.size(); ++keep) {           // cut by XLEN: the field ends inside the subfield
        CHECK(block_size_of(Bytes(bc.begin(), bc.begin() + keep)) == 0, "BC cut to %zu bytes", keep);
        CHECK(block_size_of(some + Bytes(bc.begin(), bc.begin() + keep)) == 0, "BC behind another subfield, cut to %zu bytes", keep);
    }
    {
        Bytes beyond = subfield('X', 'Y', {1, 2, 3});            // a subfield that claims more than the field holds
        beyond[2] = 200;
        CHECK(block_size_of(beyond) == 0, "SLEN beyond XLEN");
        CHECK(block_size_of(beyond + bc) == 0, "SLEN beyond XLEN hides what follows");
        beyond[2] = 0xFF; beyond[3] = 0xFF;
        CHECK(block_size_of(beyond + bc) == 0, "SLEN 65535");
    }
    // the trailer, and the little-endian readers
    {
        const Bytes t = {0x78, 0x56, 0x34, 0x12, 0xF0, 0xDE, 0xBC, 0x9A};
        const auto p = exact(t, t.size());
        const Trailer tr = read_trailer(p.get());
        CHECK(tr.crc == 0x12345678u && tr.isize == 0x9ABCDEF0u, "trailer %08x %08x", tr.crc, tr.isize);
        CHECK(le16(p.get() + 6) == 0x9ABCu && le32(p.get() + 4) == 0x9ABCDEF0u, "le16 / le32");
        const Bytes ones(8, 0xFF);
        const Trailer all = read_trailer(exact(ones, 8).get());
        CHECK(all.crc == 0xFFFFFFFFu && all.isize == 0xFFFFFFFFu, "trailer of ones");
    }
    const uint8_t magic[2] = {0x1f, 0x8b}, swapped[2] = {0x8b, 0x1f};
    CHECK(is_gzip(magic) && !is_gzip(swapped), "magic bytes");
    std::printf("ok: %ld checks\n", checks);
    return 0;
}
