// scg_library.cpp -- host-side compilation of templates and barcode pools into the flat tables
// the kernels consume.  Replaces the constructors of kaori::ScanTemplate, SimpleBarcodeSearch,
// SegmentedBarcodeSearch and the mismatch trie build (see scg_host.h for citations).
#include "scg_host.h"
#include "scg_env.h"

#include <algorithm>
#include <cstdlib>
#include <cstring>
#include <exception>
#include <mutex>
#include <thread>
#include <string>

namespace scg {

// Slots per entry of the group tables.  A wavefront repeats a probe step as long as ANY of its 64 lanes has not found its
// chain, so collisions cost far more than their per-lookup rate suggests: at 50 % load nearly every wavefront probed twice
// or more.  Small libraries, whose tables stay cache-resident anyway, get very sparse tables; for 100 k barcodes a
// quarter load is the measured optimum (MI355X: config 3 -13 % at 64 slots per entry, configs 2 and 5 -4 % at 4, +1 % at
// 8 where the tables start missing the L2).  SCG_TABLE_FACTOR overrides (tuning aid).
static uint32_t table_factor(size_t n) {
    if (env().table_factor) return static_cast<uint32_t>(env().table_factor);
    if (n <= 4096) return 64;
    if (n <= 32768) return 16;
    return 4;
}

namespace {

// code = (ascii >> 1) & 3 :  A0 C1 T2 G3
inline int base_code(char c) {
    switch (c) {
        case 'A': case 'a': return 0;
        case 'C': case 'c': return 1;
        case 'T': case 't': return 2;
        case 'G': case 'g': return 3;
        default: return -1;
    }
}

// Allowed codes of a library character in the reference's expansion order A, C, G, T
// (kaori/MismatchTrie.hpp:163-188).  Returns the count, 0 for an unknown character.
struct IupacTable {
    uint8_t n[256];
    uint8_t code[256][4];
    IupacTable() {
        std::memset(n, 0, sizeof(n));
        std::memset(code, 0, sizeof(code));
        const int A = 0, C = 1, T = 2, G = 3;
        auto def = [&](char c, std::initializer_list<int> codes) {
            for (int ch : {static_cast<int>(c), static_cast<int>(c) + ('a' - 'A')}) {
                int k = 0;
                for (int x : codes) code[ch][k++] = static_cast<uint8_t>(x);
                n[ch] = static_cast<uint8_t>(k);
            }
        };
        def('A', {A}); def('C', {C}); def('G', {G}); def('T', {T});
        def('R', {A, G}); def('Y', {C, T}); def('S', {C, G}); def('W', {A, T}); def('K', {G, T}); def('M', {A, C});
        def('B', {C, G, T}); def('D', {A, G, T}); def('H', {A, C, T}); def('V', {A, C, G});
        def('N', {A, C, G, T});
    }
};
const IupacTable& iupac() {
    static const IupacTable t;
    return t;
}
inline int iupac_codes(char c, int out[4]) {
    const IupacTable& t = iupac();
    const unsigned char u = static_cast<unsigned char>(c);
    for (int k = 0; k < 4; ++k) out[k] = t.code[u][k];
    return t.n[u];
}

const int64_t MAX_EXPANSIONS = int64_t(1) << 26;

// ---------------------------------------------------------------------------------------------
// The key classes (scg_host.h: key_class).  A class says how a key is held on the host, how it lies in a node or slot of
// the index -- WORDS 32-bit words: the key, the value at VALUE, the chain link after it, zeros up to whole uint4 -- and how
// a position group is applied to it and hashed (scg_common.h: ScgIndex; the device does the same in KeyOps).
// ---------------------------------------------------------------------------------------------
struct Narrow {                 // up to 32 bases: both 32-bit planes in one word
    typedef uint64_t Key;
    static constexpr int CLS = 0, MAXLEN = SCG_MAX_BARCODE, WORDS = 4, VALUE = 2;
    static void set_base(Key& k, int p, uint64_t code) { k |= ((code & 1) << p) | ((code >> 1) << (32 + p)); }    // plane-split (scg_common.h)
    static void put_key(uint32_t* node, Key k) { node[0] = static_cast<uint32_t>(k); node[1] = static_cast<uint32_t>(k >> 32); }
    // Turns the two position ranges of a group (as scg_big_group takes them) into the mask that masked() applies, and
    // returns what ScgIndex::segmask holds for the group: here both are the plane-split mask.
    static uint64_t group(uint64_t ranges, uint64_t mask[SCG_BIG_WORDS]) { scg_big_group(ranges, mask); mask[0] |= mask[0] << 32; return mask[0]; }
    static Key masked(Key k, const uint64_t* mask) { return k & mask[0]; }
    static uint32_t hash(Key k) { return scg_hash64(k); }
};

template<int N>
struct PlaneKey {
    uint64_t lo[N], hi[N];
    bool operator==(const PlaneKey& o) const {
        for (int w = 0; w < N; ++w) if (lo[w] != o.lo[w] || hi[w] != o.hi[w]) return false;
        return true;
    }
};
// N 64-bit words per plane: wide keys (N = 1: up to 64 bases, or several regions concatenated) and big keys
// (N = SCG_BIG_WORDS: up to 256 bases, the longest a template can be).
template<int N>
struct Planes {
    typedef PlaneKey<N> Key;
    static constexpr int CLS = N == 1 ? 1 : 2, MAXLEN = 64 * N, WORDS = N == 1 ? 8 : 20, VALUE = 4 * N;
    static void set_base(Key& k, int p, uint64_t code) { k.lo[p >> 6] |= (code & 1) << (p & 63); k.hi[p >> 6] |= (code >> 1) << (p & 63); }
    static void put_key(uint32_t* node, const Key& k) {
        for (int w = 0; w < N; ++w) {
            node[2 * w] = static_cast<uint32_t>(k.lo[w]); node[2 * w + 1] = static_cast<uint32_t>(k.lo[w] >> 32);
            node[2 * N + 2 * w] = static_cast<uint32_t>(k.hi[w]); node[2 * N + 2 * w + 1] = static_cast<uint32_t>(k.hi[w] >> 32);
        }
    }
    // wide: the 64-bit position mask itself; big: the ranges (ScgIndex::segmask)
    static uint64_t group(uint64_t ranges, uint64_t mask[SCG_BIG_WORDS]) { scg_big_group(ranges, mask); return N == 1 ? mask[0] : ranges; }
    static Key masked(Key k, const uint64_t* mask) {
        for (int w = 0; w < N; ++w) { k.lo[w] &= mask[w]; k.hi[w] &= mask[w]; }
        return k;
    }
    static uint32_t hash(const Key& k) {
        if constexpr (N == 1) return scg_hash128(k.lo[0], k.hi[0]); else return scg_hash_big(k.lo, k.hi);
    }
};

// Calls f(key) for every concrete expansion of `s` in lexicographic (A,C,G,T) order.
template<class T, class F>
void for_each_expansion(const char* s, int len, F f) {
    int cnt[T::MAXLEN], codes[T::MAXLEN][4], choice[T::MAXLEN];
    bool plain = true;
    for (int p = 0; p < len; ++p) {
        cnt[p] = iupac_codes(s[p], codes[p]);
        choice[p] = 0;
        plain &= cnt[p] == 1;
    }
    for (;;) {
        typename T::Key key = typename T::Key();
        for (int p = 0; p < len; ++p) T::set_base(key, p, static_cast<uint64_t>(codes[p][choice[p]]));
        f(key);
        if (plain) return;      // the usual library: A, C, G, T only
        int p = len - 1;
        for (; p >= 0; --p) {
            if (++choice[p] < cnt[p]) break;
            choice[p] = 0;
        }
        if (p < 0) break;
    }
}

int64_t count_expansions(const char* const* pool, int32_t n, int32_t len) {
    int64_t total = 0;
    int codes[4];
    for (int32_t i = 0; i < n; ++i) {
        int64_t m = 1;
        for (int p = 0; p < len; ++p) {
            int c = iupac_codes(pool[i][p], codes);
            if (c == 0) {
                // kaori/MismatchTrie.hpp:187
                throw Error(SCG_ERR_INVALID, std::string("unknown base '") + pool[i][p] + "' detected when constructing the trie");
            }
            m *= c;
            if (m > MAX_EXPANSIONS) break;
        }
        total += m;
        if (total > MAX_EXPANSIONS) {
            throw Error(SCG_ERR_UNSUPPORTED, "barcode pool expands to more than 2^26 concrete sequences");
        }
    }
    return total;
}

uint32_t capacity_for(int64_t entries, int slots_per_entry = 2) {
    uint64_t cap = 16;
    while (cap < static_cast<uint64_t>(entries) * static_cast<uint64_t>(slots_per_entry)) cap <<= 1;
    return static_cast<uint32_t>(cap);
}

// The pair table (build_pair_table): keys in the slots, SCG_EMPTY_KEY where free, as the device probes it.
struct Builder {
    std::vector<uint64_t>& keys;
    std::vector<int32_t>& vals;
    uint32_t mask;
    Builder(std::vector<uint64_t>& k, std::vector<int32_t>& v, uint32_t capacity) : keys(k), vals(v), mask(capacity - 1) {
        keys.assign(capacity, SCG_EMPTY_KEY);
        vals.assign(capacity, -1);
    }
    // Returns the slot holding `key`, inserting it (with val) if absent; *existed tells which.
    uint32_t upsert(uint64_t key, int32_t val, bool* existed) {
        uint32_t h = scg_hash64(key) & mask;
        for (;;) {
            if (keys[h] == key) { *existed = true; return h; }
            if (keys[h] == SCG_EMPTY_KEY) { keys[h] = key; vals[h] = val; *existed = false; return h; }
            h = (h + 1) & mask;
        }
    }
};

// The distinct keys of a pool in the order met, with an exact host-only map from a key to its number in that order: open
// addressing over the numbers, half full at most, so that no key value has to stand for a free slot.
template<class T>
struct KeySet {
    std::vector<typename T::Key> keys;
    std::vector<int32_t> slots;
    explicit KeySet(int64_t total) : slots(capacity_for(total), -1) { keys.reserve(static_cast<size_t>(total)); }
    // Returns the number of `key`, appending it if absent; *existed tells which.
    int32_t upsert(const typename T::Key& key, bool* existed) {
        const uint32_t mask = static_cast<uint32_t>(slots.size()) - 1;
        for (uint32_t h = T::hash(key) & mask;; h = (h + 1) & mask) {
            const int32_t e = slots[h];
            if (e < 0) {
                slots[h] = static_cast<int32_t>(keys.size());
                keys.push_back(key);
                *existed = false;
                return slots[h];
            }
            if (keys[e] == key) { *existed = true; return e; }
        }
    }
};

[[noreturn]] void throw_duplicate(int32_t a, int32_t b) {
    // kaori/MismatchTrie.hpp:119-122
    throw Error(SCG_ERR_INVALID, "duplicate sequences detected (" + std::to_string(a + 1) + ", " + std::to_string(b + 1) + ") when constructing the trie");
}

} // namespace

HostTemplate parse_template(const char* constant, int strand) {
    size_t len = std::strlen(constant);
    if (len > SCG_MAX_TEMPLATE) {
        // src/count_single_barcodes.cpp:46
        throw Error(SCG_ERR_INVALID, "lacking compile-time support for constant regions longer than 256 bp");
    }
    HostTemplate out;
    std::memset(&out.t, 0, sizeof(out.t));
    out.fwd = (strand != 1);   // src/utils.cpp:33-41: 0 forward, 1 reverse, anything else both
    out.rev = (strand != 0);   // kaori/utils.hpp:33-39
    ScgTemplate& t = out.t;
    t.len = static_cast<int32_t>(len);

    int L = t.len;
    int nreg = 0, nconst = 0;
    int starts[SCG_MAX_TEMPLATE], ends[SCG_MAX_TEMPLATE];
    for (int i = 0; i < L; ++i) {
        char b = constant[i];
        if (b == '-') {
            if (nreg && ends[nreg - 1] == i) {
                ++ends[nreg - 1];
            } else {
                starts[nreg] = i; ends[nreg] = i + 1; ++nreg;
            }
        } else {
            int c = base_code(b);
            if (c < 0) {
                if (out.fwd) {
                    throw Error(SCG_ERR_INVALID, std::string("unknown base '") + b + "'");          // kaori/utils.hpp:156-158
                } else {
                    throw Error(SCG_ERR_INVALID, std::string("cannot complement unknown base '") + b + "'");  // :117
                }
            }
            t.fpos[nconst] = static_cast<uint8_t>(i);
            t.fcode[nconst] = static_cast<uint8_t>(c);
            ++nconst;
        }
    }
    t.nconst = nconst;
    t.nreg = nreg;
    // reverse-complemented template: position i of it is the complement of position L-1-i
    for (int k = 0; k < nconst; ++k) {
        int src = nconst - 1 - k;
        t.rpos[k] = static_cast<uint8_t>(L - 1 - t.fpos[src]);
        t.rcode[k] = static_cast<uint8_t>(t.fcode[src] ^ 2);
    }
    // Callers reject any template whose region count is not the one they expect, so only
    // region counts the engine can use are materialised.
    if (nreg <= SCG_MAX_REGIONS) {
        for (int r = 0; r < nreg; ++r) {
            t.fstart[r] = starts[r];
            t.flen[r] = ends[r] - starts[r];
            int src = nreg - 1 - r;             // kaori/ScanTemplate.hpp:82-94
            t.rstart[r] = L - ends[src];
            t.rlen[r] = ends[src] - starts[src];
        }
    }
    return out;
}

int pool_length(const char* const* pool, int32_t n) {
    // src/utils.cpp:5-23
    size_t size = 0;
    for (int32_t i = 0; i < n; ++i) {
        size_t cur = std::strlen(pool[i]);
        if (i == 0) {
            size = cur;
        } else if (cur != size) {
            throw Error(SCG_ERR_INVALID, "variable regions should all have the same length (" + std::to_string(size) + ")");
        }
    }
    return static_cast<int>(size);
}

namespace {

// fn(0) .. fn(n - 1), each on its own thread (n <= 6 position groups).
template<class F>
void for_each_group(int n, F fn) {
    std::exception_ptr err;
    std::mutex mu;
    auto guarded = [&](int i) {
        try {
            fn(i);
        } catch (...) {
            std::lock_guard<std::mutex> g(mu);
            if (!err) err = std::current_exception();
        }
    };
    std::vector<std::thread> th;
    for (int i = 1; i < n; ++i) th.emplace_back(guarded, i);
    if (n > 0) guarded(0);
    for (auto& t : th) t.join();
    if (err) std::rethrow_exception(err);
}

// Lays the concrete entries (key, value) out as a segment index (scg_common.h: ScgIndex).
template<class T>
void finish_index(HostIndex& X, const std::vector<typename T::Key>& keys, const std::vector<int32_t>& vals, int32_t len, int max_mm) {
    constexpr int NW = T::WORDS, NEXT = T::VALUE + 1;
    const size_t n = keys.size();
    X.wide = T::CLS;
    X.len = len;
    X.n_entries = static_cast<int32_t>(n);
    // position groups (see ScgIndex): one or two of `parts` equal slices of the barcode, each a range [a, b) of positions
    // packed as a | b << 16, the second 32 bits up (scg_big_group)
    auto slice = [&](int part, int parts) -> uint64_t {
        const uint64_t a = static_cast<uint64_t>(static_cast<int64_t>(part) * len / parts);
        const uint64_t b = static_cast<uint64_t>(static_cast<int64_t>(part + 1) * len / parts);
        return a | (b << 16);
    };
    std::vector<uint64_t> groups;
    if (max_mm == 0) {
        groups.push_back(slice(0, 1));
        X.nwalk[0] = X.nwalk[1] = X.nwalk[2] = X.nwalk[3] = 1;
    } else if (max_mm == 1) {
        groups.push_back(slice(0, 2));
        groups.push_back(slice(1, 2));
        X.nwalk[0] = 1; X.nwalk[1] = X.nwalk[2] = X.nwalk[3] = 2;
    } else if (max_mm == 2) {
        static const int pairs[6][2] = {{0, 1}, {2, 3}, {0, 2}, {1, 3}, {0, 3}, {1, 2}};
        for (auto& pr : pairs) groups.push_back(slice(pr[0], 4) | (slice(pr[1], 4) << 32));
        X.nwalk[0] = 1; X.nwalk[1] = 2; X.nwalk[2] = X.nwalk[3] = 6;
    } else if (max_mm == 3) {
        for (int q = 0; q < 4; ++q) groups.push_back(slice(q, 4));
        X.nwalk[0] = 1; X.nwalk[1] = 2; X.nwalk[2] = 3; X.nwalk[3] = 4;
    }                          // wider budgets: no tables (nseg = 0), dense scans of the node array
    const int nseg = static_cast<int>(groups.size());
    X.nseg = nseg;
    const int ncopies = nseg > 0 ? nseg : 1;
    X.nodes.resize(static_cast<size_t>(ncopies) * n * NW);      // (zeros: the padding words stay so)
    for (int c = 0; c < ncopies; ++c) {
        uint32_t* node = X.nodes.data() + static_cast<size_t>(c) * n * NW;
        for (size_t e = 0; e < n; ++e) {
            T::put_key(node + NW * e, keys[e]);
            node[NW * e + T::VALUE] = static_cast<uint32_t>(vals[e]);
            node[NW * e + NEXT] = 0xFFFFFFFFu;      // chain end until linked below
        }
    }
    if (nseg == 0) return;

    // One table per group, open addressing with linear probing, one slot count for all (load: table_factor).  Entries
    // agreeing on the group's positions form a chain in ascending entry order whose head sits in the slot itself: going
    // through the entries back to front, each either claims a free slot or becomes the new head of the chain it finds.
    // The groups are independent and are built side by side (the build overlaps the first window of a file only).
    uint32_t cap = 16;
    while (cap < n * table_factor(n)) cap <<= 1;
    X.slot_mask = cap - 1;
    X.tables.resize(static_cast<size_t>(nseg) * cap * NW);
    uint64_t masks[SCG_MAX_SEGMENTS][SCG_BIG_WORDS];
    for (int sgm = 0; sgm < nseg; ++sgm) X.segmask[sgm] = T::group(groups[sgm], masks[sgm]);
    for_each_group(nseg, [&](int sgm) {
        const uint64_t* mask = masks[sgm];
        const uint32_t slot_mask = X.slot_mask;
        uint32_t* node = X.nodes.data() + static_cast<size_t>(sgm) * n * NW;
        uint32_t* table = X.tables.data() + static_cast<size_t>(sgm) * cap * NW;
        std::vector<int32_t> placed(cap, -1);
        for (size_t i = n; i-- > 0;) {
            const typename T::Key sk = T::masked(keys[i], mask);
            uint32_t pos = T::hash(sk) & slot_mask;
            for (;;) {
                const int32_t e = placed[pos];
                if (e < 0) { placed[pos] = static_cast<int32_t>(i); break; }
                if (T::masked(keys[e], mask) == sk) {
                    node[NW * i + NEXT] = static_cast<uint32_t>(e);
                    placed[pos] = static_cast<int32_t>(i);
                    break;
                }
                pos = (pos + 1) & slot_mask;
            }
        }
        for (uint32_t pos = 0; pos < cap; ++pos) {
            const int32_t e = placed[pos];
            uint32_t* slot = table + static_cast<size_t>(NW) * pos;
            if (e < 0) slot[NEXT] = SCG_SLOT_EMPTY;      // (the other words are zero)
            else for (int w = 0; w < NW; ++w) slot[w] = node[NW * static_cast<size_t>(e) + w];
        }
    });
}

// The index of a pool in key class T.  Without `expansions`, value = barcode index and a sequence met twice is an error;
// with it, value = uid, the sequence's number among the distinct ones in the order met, and expansions[i] lists barcode i's.
template<class T>
HostIndex build(const char* const* pool, int32_t n, int32_t len, int max_mm, std::vector<std::vector<int32_t> >* expansions,
                std::vector<uint64_t>* uid_keys) {
    if (len > T::MAXLEN) {
        throw Error(SCG_ERR_UNSUPPORTED, "variable regions longer than " + std::to_string(T::MAXLEN) + (T::CLS ? " bp in total" : " bp") +
                                         " are not supported by this engine (got " + std::to_string(len) + ")");
    }
    const int64_t total = count_expansions(pool, n, len);
    KeySet<T> seen(total);
    std::vector<int32_t> vals;
    vals.reserve(static_cast<size_t>(total));
    if (expansions) expansions->assign(n, std::vector<int32_t>());
    for (int32_t i = 0; i < n; ++i) {
        for_each_expansion<T>(pool[i], len, [&](const typename T::Key& key) {
            bool existed;
            const int32_t e = seen.upsert(key, &existed);
            if (expansions) (*expansions)[i].push_back(e);
            else if (existed) throw_duplicate(vals[e], i);
            if (!existed) vals.push_back(expansions ? e : i);
        });
    }
    HostIndex X;
    finish_index<T>(X, seen.keys, vals, len, max_mm);
    if constexpr (T::CLS == 0) {
        if (uid_keys) *uid_keys = std::move(seen.keys);
    }
    return X;
}

HostIndex build_class(int cls, const char* const* pool, int32_t n, int32_t len, int max_mm, std::vector<std::vector<int32_t> >* expansions,
                      std::vector<uint64_t>* uid_keys) {
    if (cls == 0) return build<Narrow>(pool, n, len, max_mm, expansions, uid_keys);
    return cls == 1 ? build<Planes<1> >(pool, n, len, max_mm, expansions, uid_keys) : build<Planes<SCG_BIG_WORDS> >(pool, n, len, max_mm, expansions, uid_keys);
}

} // namespace

HostIndex build_index(const char* const* pool, int32_t n, int32_t len, int max_mm, int cls) {
    return build_class(cls, pool, n, len, max_mm, nullptr, nullptr);
}

HostIndex build_uid_index(const char* const* pool, int32_t n, int32_t len, int max_mm, int cls,
                          std::vector<std::vector<int32_t> >& expansions, std::vector<uint64_t>& uid_keys) {
    uid_keys.clear();
    return build_class(cls, pool, n, len, max_mm, &expansions, &uid_keys);
}

HostPairTable build_pair_table(const std::vector<std::vector<int32_t> >& exp1, const std::vector<uint64_t>& uid_keys1,
                               const std::vector<std::vector<int32_t> >& exp2, const std::vector<uint64_t>& uid_keys2) {
    HostPairTable P;
    int64_t total = 0;
    for (size_t i = 0; i < exp1.size(); ++i) {
        total += static_cast<int64_t>(exp1[i].size()) * static_cast<int64_t>(exp2[i].size());
        if (total > MAX_EXPANSIONS) {
            throw Error(SCG_ERR_UNSUPPORTED, "barcode pairs expand to more than 2^26 concrete sequences");
        }
    }
    Builder B(P.keys, P.vals, capacity_for(total, 4));      // this one is probed by the device: a quarter full
    P.mask = B.mask;
    for (size_t i = 0; i < exp1.size(); ++i) {
        // concatenated expansions in lexicographic order: first barcode major
        for (int32_t u1 : exp1[i]) {
            for (int32_t u2 : exp2[i]) {
                uint64_t key = (static_cast<uint64_t>(static_cast<uint32_t>(u1)) << 32) | static_cast<uint32_t>(u2);
                bool existed;
                uint32_t slot = B.upsert(key, static_cast<int32_t>(i), &existed);
                if (existed) throw_duplicate(P.vals[slot], static_cast<int32_t>(i));
                if (!uid_keys1.empty() && !uid_keys2.empty()) {      // (wide pools pass none: they have no dense-scan fallback)
                    P.list_key1.push_back(uid_keys1[u1]);
                    P.list_key2.push_back(uid_keys2[u2]);
                }
                P.list_vals.push_back(static_cast<int32_t>(i));
            }
        }
    }
    P.n_entries = static_cast<int32_t>(P.list_vals.size());
    return P;
}

ScgScan build_scan(const ScgTemplate& t, int max_mm) {
    ScgScan sc;
    std::memset(&sc, 0, sizeof(sc));
    sc.len = t.len;
    sc.nreg = t.nreg;
    for (int r = 0; r < SCG_MAX_REGIONS; ++r) {
        sc.fstart[r] = t.fstart[r];
        sc.rstart[r] = t.rstart[r];
        sc.flen[r] = t.flen[r];
        sc.rlen[r] = t.rlen[r];
    }
    for (int k = 0; k < t.nconst; ++k) {
        int fp = t.fpos[k], rp = t.rpos[k];
        sc.fmask[fp >> 5] |= 1u << (fp & 31);
        sc.fplane0[fp >> 5] |= static_cast<uint32_t>(t.fcode[k] & 1) << (fp & 31);
        sc.fplane1[fp >> 5] |= static_cast<uint32_t>(t.fcode[k] >> 1) << (fp & 31);
        sc.rmask[rp >> 5] |= 1u << (rp & 31);
        sc.rplane0[rp >> 5] |= static_cast<uint32_t>(t.rcode[k] & 1) << (rp & 31);
        sc.rplane1[rp >> 5] |= static_cast<uint32_t>(t.rcode[k] >> 1) << (rp & 31);
    }
    // k + 1 disjoint groups of constant positions for a budget of k mismatches; with fewer than
    // k + 1 constant bases (or k + 1 > SCG_MAX_SEEDS) no filter is possible and every position is
    // a candidate.
    // (9 of the SCG_SEED_LEN = 10 bases a seed may have: measured -1 % on config 2, -2 % on config 3, neutral elsewhere;
    // 8 costs +11 %: a false candidate then precedes the true one in a third of the wavefronts)
    static_assert(Env::SEED_LEN == SCG_SEED_LEN, "scg_env.h bounds SCG_SEED_MAX by the seed length");
    const int seed_max = env().seed_max;         // SCG_SEED_LEN - 1 unless SCG_SEED_MAX says otherwise (tuning aid)
    auto fill = [&](ScgSeeds& S, const uint8_t* pos, const uint8_t* code) {
        int want = max_mm + 1;
        if (want > SCG_MAX_SEEDS || t.nconst < want) {
            S.nseeds = 0;
            return;
        }
        // Any k + 1 disjoint groups of constant positions satisfy the pigeonhole argument.  Candidates: runs of up to
        // seed_max constant positions (consecutive in the list of constant positions) that stay inside one block of 32
        // template positions -- the scanners take a shifted plane word from two adjacent words, and blocks 0 and 1 keep
        // the compact scanner applicable.  The longest runs win (fewest false candidates), earlier ones first.
        struct Run { int first, n, blk; };
        std::vector<Run> runs;
        for (int k = 0; k < t.nconst;) {
            const int blk = pos[k] >> 5;
            int n = 1;
            while (k + n < t.nconst && n < seed_max && (pos[k + n] >> 5) == blk) ++n;
            runs.push_back(Run{k, n, blk});
            k += n;
        }
        if (static_cast<int>(runs.size()) < want) {      // fewer runs than seeds: split the longest until there are enough
            while (static_cast<int>(runs.size()) < want) {
                size_t big = 0;
                for (size_t i = 1; i < runs.size(); ++i) if (runs[i].n > runs[big].n) big = i;
                if (runs[big].n < 2) break;
                const Run r = runs[big];
                runs[big] = Run{r.first, r.n / 2, r.blk};
                runs.insert(runs.begin() + static_cast<long>(big) + 1, Run{r.first + r.n / 2, r.n - r.n / 2, r.blk});
            }
        }
        if (static_cast<int>(runs.size()) < want) { S.nseeds = 0; return; }
        std::stable_sort(runs.begin(), runs.end(), [](const Run& x, const Run& y) { return x.n > y.n; });
        runs.resize(static_cast<size_t>(want));
        std::sort(runs.begin(), runs.end(), [](const Run& x, const Run& y) { return x.first < y.first; });
        S.nseeds = want;
        for (int i = 0; i < want; ++i) {
            const int a = runs[static_cast<size_t>(i)].first;
            ScgSeed sd;
            std::memset(&sd, 0, sizeof(sd));
            sd.len = runs[static_cast<size_t>(i)].n;
            sd.blk = runs[static_cast<size_t>(i)].blk;
            for (int c = 0; c < 4; ++c) {
                uint8_t steps[64];
                int ns = 0;
                for (int j = 0; j < sd.len; ++j) {
                    if (code[a + j] != c) continue;
                    steps[ns++] = static_cast<uint8_t>(pos[a + j] - 32 * sd.blk);      // offset within the block, < 32
                }
                if (ns & 1) { steps[ns] = steps[ns - 1]; ++ns; }      // even step count: the compact scanner folds bases in pairs (a repeated AND is a no-op)
                for (int k = 0; k < ns; ++k) sd.walk[c].w[k >> 2] |= static_cast<uint32_t>(steps[k]) << (8 * (k & 3));
                sd.nsteps |= static_cast<uint32_t>(ns) << (8 * c);
            }
            S.seed[i] = sd;
        }
    };
    fill(sc.fseeds, t.fpos, t.fcode);
    fill(sc.rseeds, t.rpos, t.rcode);
    // The compact kernels keep only the candidate words and read shifted plane words straight from the planes: valid
    // while every seed lies in block 0 or 1.
    sc.compact_ok = 1;
    for (const ScgSeeds* S : {&sc.fseeds, &sc.rseeds}) {
        for (int i = 0; i < S->nseeds; ++i) if (S->seed[i].blk > 1) sc.compact_ok = 0;
    }
    return sc;
}

} // namespace scg
