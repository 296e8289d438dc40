// scg_gzip.h -- the gzip container (RFC 1952), once: the magic bytes, a member's header and trailer, BGZF's size
// subfield, and the look-up of libdeflate that the host's gzip readers share.  The DEFLATE stream inside a member is
// scg_inflate.h's.  Plain host C++, nothing from HIP: tests/gzip_container_harness.cpp runs the parsers on exact-size
// buffers under AddressSanitizer, and tests/pgzip_harness.cpp links scg_pgzip.cpp alone.
//
// The parsers say what a header IS; what a reader TAKES is its own policy, one visible line at each call site (the chunked
// decoders leave a header CRC and reserved flags to zlib, the device BGZF path takes FEXTRA only, ...).
#ifndef SCG_GZIP_H
#define SCG_GZIP_H

#include <cstddef>
#include <cstdint>
#include <cstdlib>
#include <dlfcn.h>
#include <initializer_list>

#include "scg_env.h"

namespace scg {
namespace gz {

// What the reference tells a gzip file by (byteme/magic_numbers.hpp:19-22).
inline bool is_gzip(const unsigned char* two_bytes) { return two_bytes[0] == 0x1f && two_bytes[1] == 0x8b; }

inline uint32_t le16(const uint8_t* p) { return p[0] | (static_cast<uint32_t>(p[1]) << 8); }
inline uint32_t le32(const uint8_t* p) { return le16(p) | (le16(p + 2) << 16); }

enum : uint8_t { FHCRC = 2, FEXTRA = 4, FNAME = 8, FCOMMENT = 16 };      // (bits 5-7: reserved)

struct MemberHeader {
    uint8_t flags;
    size_t extra_at, extra_len;      // the extra field's bytes (FEXTRA; else 0, 0), as offsets into data
    size_t payload;                  // where the DEFLATE stream begins
};

// The member header at data[off ...) of data[0 .. size): true if it has the magic bytes and CM = 8 (deflate) and every
// field its flags announce -- extra field, name, comment, header CRC -- lies within `size`.  Reads nothing beyond `size`.
// `walk`: the fields to walk (BGZF members are told by their extra field alone: `payload` then lies behind that).
inline bool parse_member_header(const uint8_t* data, size_t size, size_t off, MemberHeader& h, uint8_t walk = 0xFF) {
    if (off > size || size - off < 10 || !is_gzip(data + off) || data[off + 2] != 8) return false;
    h.flags = data[off + 3];
    const uint8_t fields = h.flags & walk;
    h.extra_at = h.extra_len = 0;
    size_t p = off + 10;
    if (fields & FEXTRA) {
        if (size - p < 2) return false;
        h.extra_len = le16(data + p);
        p += 2;
        h.extra_at = p;
        if (size - p < h.extra_len) return false;
        p += h.extra_len;
    }
    for (int field : {FNAME, FCOMMENT}) {                       // zero-terminated
        if (fields & field) {
            while (p < size && data[p]) ++p;
            if (p == size) return false;
            ++p;
        }
    }
    if (fields & FHCRC) {
        if (size - p < 2) return false;
        p += 2;
    }
    h.payload = p;
    return true;
}

// BGZF (the SAM/BAM specification, written by bgzip): the member's whole size from the 'BC' subfield of its extra field,
// or 0 if there is none of the right form within the field.
inline size_t bgzf_block_size(const uint8_t* data, const MemberHeader& h) {
    const uint8_t* x = data + h.extra_at;
    for (size_t at = 0; at + 4 <= h.extra_len;) {
        const size_t slen = le16(x + at + 2);
        if (x[at] == 'B' && x[at + 1] == 'C' && slen == 2 && at + 6 <= h.extra_len) return le16(x + at + 4) + size_t(1);
        at += 4 + slen;
    }
    return 0;
}

// The eight bytes behind a member's DEFLATE stream.
struct Trailer { uint32_t crc, isize; };
inline Trailer read_trailer(const uint8_t* p) { return Trailer{le32(p), le32(p + 4)}; }

// libdeflate (whole-buffer DEFLATE at 2-3 x zlib's inflate, CRC-32 by carry-less multiplication at ~10 GB/s) is part of
// the image as a shared library without headers: looked up at run time, once, and never unloaded.  Null when the library
// is absent or SCG_LIBDEFLATE=0 (asked at every call, before any look-up); a function the library lacks is null.
struct Libdeflate {
    void* (*alloc)() = nullptr;
    void (*release)(void*) = nullptr;
    int (*gzip_ex)(void*, const void*, size_t, void*, size_t, size_t*, size_t*) = nullptr;      // null unless all three are there
    uint32_t (*crc32)(uint32_t, const void*, size_t) = nullptr;
};
inline const Libdeflate* libdeflate() {
    if (!env().libdeflate) return nullptr;
    static const Libdeflate* const found = []() -> const Libdeflate* {
        void* h = ::dlopen("libdeflate.so.0", RTLD_NOW | RTLD_LOCAL);
        if (!h) return nullptr;
        Libdeflate* L = new Libdeflate;
        L->alloc = reinterpret_cast<decltype(L->alloc)>(::dlsym(h, "libdeflate_alloc_decompressor"));
        L->release = reinterpret_cast<decltype(L->release)>(::dlsym(h, "libdeflate_free_decompressor"));
        L->gzip_ex = reinterpret_cast<decltype(L->gzip_ex)>(::dlsym(h, "libdeflate_gzip_decompress_ex"));
        if (!L->alloc || !L->release || !L->gzip_ex) L->alloc = nullptr, L->release = nullptr, L->gzip_ex = nullptr;
        L->crc32 = reinterpret_cast<decltype(L->crc32)>(::dlsym(h, "libdeflate_crc32"));
        return L;
    }();
    return found;
}

}  // namespace gz
}  // namespace scg

#endif
