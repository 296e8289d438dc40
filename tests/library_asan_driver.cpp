// library_asan_driver.cpp -- the index builder (csrc/scg_library.cpp: IUPAC expansion, duplicate detection, chains and
// tables of every position group, built by one thread per group) checked on the host, in every key class.
//
//   <seed> <rounds> <wider rounds>   under AddressSanitizer + UBSan (tests/test_ingest_asan.py): random pools, <rounds> of
//                     narrow keys, then <wider rounds> each of wide and big keys; every entry of the index and of the uid index must be found again the way the device looks for it -- hash of its group key,
//                     linear probing to the slot whose head shares the key, then along the chain -- and small pools are
//                     compared with a naive expansion written here.
//   digest            one FNV-1a digest per fixed seeded pool over everything the builder hands out, or the error it
//                     raises (tests/test_ingest_asan.py compares with tests/golden/index_digests.txt).
//   time              minimum build time of four pools over some repetitions (profiles/index_build_time.txt).
#include "scg_host.h"

#include <algorithm>
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
#include <random>
#include <set>
#include <string>
#include <vector>

using namespace scg;

typedef std::vector<std::vector<int32_t> > Expansions;

// ---- the builders under test ----

static HostIndex index_of(const std::vector<const char*>& p, int len, int mm, int cls) {
    return build_index(p.data(), static_cast<int32_t>(p.size()), len, mm, cls);
}

static HostIndex uid_index_of(const std::vector<const char*>& p, int len, int mm, int cls, Expansions& exp, std::vector<uint64_t>& uid_keys) {
    return build_uid_index(p.data(), static_cast<int32_t>(p.size()), len, mm, cls, exp, uid_keys);
}

// ---- an index as the device reads it (scg_common.h: ScgIndex) ----

struct Planes { uint64_t lo[SCG_BIG_WORDS], hi[SCG_BIG_WORDS]; };

static bool same(const Planes& a, const Planes& b) { return std::memcmp(&a, &b, sizeof(Planes)) == 0; }
static int node_words(const HostIndex& X) { return X.wide == 0 ? 4 : (X.wide == 1 ? 8 : 20); }
static int value_word(const HostIndex& X) { return X.wide == 0 ? 2 : (X.wide == 1 ? 4 : 4 * SCG_BIG_WORDS); }     // the chain link follows it

static Planes planes_of(const HostIndex& X, const uint32_t* node) {
    Planes k;
    std::memset(&k, 0, sizeof(k));
    if (X.wide == 0) { k.lo[0] = node[0]; k.hi[0] = node[1]; return k; }
    const int nw = X.wide == 1 ? 1 : SCG_BIG_WORDS;
    for (int w = 0; w < nw; ++w) {
        k.lo[w] = (static_cast<uint64_t>(node[2 * w + 1]) << 32) | node[2 * w];
        k.hi[w] = (static_cast<uint64_t>(node[2 * nw + 2 * w + 1]) << 32) | node[2 * nw + 2 * w];
    }
    return k;
}

// The positions of group s as a mask over both planes.
static Planes group_mask(const HostIndex& X, int s) {
    Planes m;
    std::memset(&m, 0, sizeof(m));
    if (X.wide == 0) { m.lo[0] = X.segmask[s] & 0xFFFFFFFFull; m.hi[0] = X.segmask[s] >> 32; }
    else if (X.wide == 1) { m.lo[0] = m.hi[0] = X.segmask[s]; }
    else { scg_big_group(X.segmask[s], m.lo); std::memcpy(m.hi, m.lo, sizeof(m.hi)); }
    return m;
}

static Planes masked(Planes k, const Planes& m) {
    for (int w = 0; w < SCG_BIG_WORDS; ++w) { k.lo[w] &= m.lo[w]; k.hi[w] &= m.hi[w]; }
    return k;
}

static uint32_t group_hash(const HostIndex& X, const Planes& k) {
    if (X.wide == 0) return scg_hash64((k.hi[0] << 32) | k.lo[0]);
    return X.wide == 1 ? scg_hash128(k.lo[0], k.hi[0]) : scg_hash_big(k.lo, k.hi);
}

static std::string sequence_of(const HostIndex& X, const uint32_t* node) {
    const Planes k = planes_of(X, node);
    const int per = X.wide == 0 ? 32 : 64;
    std::string s(static_cast<size_t>(X.len), '?');
    for (int p = 0; p < X.len; ++p) s[p] = "ACTG"[((k.lo[p / per] >> (p % per)) & 1) | (((k.hi[p / per] >> (p % per)) & 1) << 1)];
    return s;
}

static bool reachable(const HostIndex& X, int s, const Planes& mask, size_t e) {
    const size_t n = static_cast<size_t>(X.n_entries), nw = static_cast<size_t>(node_words(X));
    const int vw = value_word(X);
    const uint32_t cap = X.slot_mask + 1;
    const uint32_t* node = X.nodes.data() + static_cast<size_t>(s) * n * nw;
    const uint32_t* table = X.tables.data() + static_cast<size_t>(s) * cap * nw;
    const Planes key = planes_of(X, node + nw * e), sk = masked(key, mask);
    uint32_t pos = group_hash(X, sk) & X.slot_mask;
    for (uint32_t step = 0; step <= cap; ++step, pos = (pos + 1) & X.slot_mask) {
        const uint32_t* slot = table + nw * pos;
        if (slot[vw + 1] == SCG_SLOT_EMPTY) return false;
        const Planes hk = planes_of(X, slot);
        if (!same(masked(hk, mask), sk)) continue;
        // the slot holds a copy of the chain's head; the chain continues in the node array
        if (same(hk, key) && slot[vw] == node[nw * e + vw]) return true;
        for (uint32_t nx = slot[vw + 1]; nx != 0xFFFFFFFFu; nx = node[nw * nx + vw + 1]) {
            if (nx >= n) return false;
            if (nx == e) return true;
        }
        return false;
    }
    return false;
}

static bool all_reachable(const HostIndex& X, const char* what, const char* where) {
    for (int s = 0; s < X.nseg; ++s) {
        const Planes mask = group_mask(X, s);
        for (size_t e = 0; e < static_cast<size_t>(X.n_entries); ++e) {
            if (!reachable(X, s, mask, e)) { fprintf(stderr, "%s: entry %zu not reachable through table %d (%s)\n", what, e, s, where); return false; }
        }
    }
    return true;
}

// ---- the naive expansion: concrete sequences of a barcode in A, C, G, T lexicographic order ----

static const char* allowed(char c) {
    switch (c) {
        case 'A': return "A"; case 'C': return "C"; case 'G': return "G"; case 'T': return "T";
        case 'R': return "AG"; case 'Y': return "CT"; case 'S': return "CG"; case 'W': return "AT"; case 'K': return "GT"; case 'M': return "AC";
        case 'B': return "CGT"; case 'D': return "AGT"; case 'H': return "ACT"; case 'V': return "ACG"; case 'N': return "ACGT";
    }
    return "";
}

static void expand(const std::string& s, size_t p, std::string& cur, std::vector<std::string>& out) {
    if (p == s.size()) { out.push_back(cur); return; }
    for (const char* a = allowed(s[p]); *a; ++a) { cur[p] = *a; expand(s, p + 1, cur, out); }
}

// Entry e of X must be (seqs[e], vals[e]), in the first node copy.
static bool same_entries(const HostIndex& X, const std::vector<std::string>& seqs, const std::vector<int32_t>& vals, const char* what, const char* where) {
    if (static_cast<size_t>(X.n_entries) != seqs.size()) { fprintf(stderr, "%s: %d entries, expected %zu (%s)\n", what, X.n_entries, seqs.size(), where); return false; }
    for (size_t e = 0; e < seqs.size(); ++e) {
        const uint32_t* node = X.nodes.data() + static_cast<size_t>(node_words(X)) * e;
        if (sequence_of(X, node) != seqs[e] || node[value_word(X)] != static_cast<uint32_t>(vals[e])) {
            fprintf(stderr, "%s: entry %zu is (%s, %u), expected (%s, %d) (%s)\n", what, e, sequence_of(X, node).c_str(), node[value_word(X)], seqs[e].c_str(), vals[e], where);
            return false;
        }
    }
    return true;
}

static bool check_pool(const std::vector<std::string>& pool, int len, int mm, int cls, const char* where, long& entries) {
    std::vector<const char*> p;
    for (auto& s : pool) p.push_back(s.c_str());
    const bool naive = pool.size() <= 600;
    std::vector<std::string> seqs, useqs;            // entries of the index / of the uid index, in order
    std::vector<int32_t> vals, uvals;
    Expansions uexp(pool.size());
    bool duplicate = false;
    if (naive) {
        std::map<std::string, int32_t> uid_of;
        for (size_t i = 0; i < pool.size(); ++i) {
            std::vector<std::string> mine;
            std::string cur = pool[i];
            expand(pool[i], 0, cur, mine);
            for (auto& s : mine) {
                auto ins = uid_of.insert(std::make_pair(s, static_cast<int32_t>(useqs.size())));
                if (ins.second) { useqs.push_back(s); uvals.push_back(ins.first->second); } else duplicate = true;
                uexp[i].push_back(ins.first->second);
                seqs.push_back(s);
                vals.push_back(static_cast<int32_t>(i));
            }
        }
    }
    try {
        const HostIndex X = index_of(p, len, mm, cls);
        if (X.wide != cls || !all_reachable(X, "index", where)) return false;
        if (naive && (duplicate || !same_entries(X, seqs, vals, "index", where))) {
            if (duplicate) fprintf(stderr, "index: duplicate sequences went unnoticed (%s)\n", where);
            return false;
        }
        entries += X.n_entries;
    } catch (const Error&) {
        // two barcodes whose expansions collide: the reference's "duplicate sequences" error, fine
        if (naive && !duplicate) { fprintf(stderr, "index: error without duplicate sequences (%s)\n", where); return false; }
    }
    Expansions exp;
    std::vector<uint64_t> uid_keys;
    const HostIndex U = uid_index_of(p, len, mm, cls, exp, uid_keys);
    if (U.wide != cls || !all_reachable(U, "uid index", where)) return false;
    if (cls == 0 && uid_keys.size() != static_cast<size_t>(U.n_entries)) { fprintf(stderr, "uid index: %zu uid keys (%s)\n", uid_keys.size(), where); return false; }
    for (size_t u = 0; u < uid_keys.size(); ++u) {
        if (uid_keys[u] != ((static_cast<uint64_t>(U.nodes[4 * u + 1]) << 32) | U.nodes[4 * u])) { fprintf(stderr, "uid index: uid key %zu (%s)\n", u, where); return false; }
    }
    if (naive && (!same_entries(U, useqs, uvals, "uid index", where) || exp != uexp)) {
        if (exp != uexp) fprintf(stderr, "uid index: expansions differ (%s)\n", where);
        return false;
    }
    entries += U.n_entries;
    return true;
}

static int random_rounds(uint64_t seed, int rounds, int other_rounds) {
    std::mt19937_64 rng(seed);
    long entries = 0;
    int pools = 0;
    for (int cls = 0; cls < 3; ++cls) {
        for (int r = 0; r < (cls == 0 ? rounds : other_rounds); ++r, ++pools) {
            const int len = cls == 0 ? 4 + static_cast<int>(rng() % 29) : (cls == 1 ? 33 + static_cast<int>(rng() % 32) : 65 + static_cast<int>(rng() % 192));
            int n = 1 + static_cast<int>(rng() % (r % 5 == 0 ? (cls == 0 ? 40000 : 4000) : 600));
            if (len < 10) n = std::min(n, (1 << (2 * len)) / 4);                  // (there are only 4^len sequences)
            const int mm = static_cast<int>(rng() % 4);
            std::set<std::string> seen;
            std::vector<std::string> pool;
            while (static_cast<int>(pool.size()) < n) {
                std::string s(len, 'A');
                for (auto& c : s) c = "ACGT"[rng() % 4];
                if (rng() % 50 == 0) s[rng() % len] = "RYSWKMN"[rng() % 7];      // an ambiguous base now and then
                if (seen.insert(s).second) pool.push_back(s);
                if (seen.size() > 100000) break;
            }
            char where[96];
            snprintf(where, sizeof(where), "class %d round %d: n %d len %d mm %d", cls, r, n, len, mm);
            if (!check_pool(pool, len, mm, cls, where, entries)) return 1;
        }
    }
    printf("ok: %d pools, %ld entries reachable through every table\n", pools, entries);
    return 0;
}

// ---- digests ----

struct Fnv {
    uint64_t h = 0xCBF29CE484222325ull;
    void bytes(const void* p, size_t n) {
        const unsigned char* b = static_cast<const unsigned char*>(p);
        for (size_t i = 0; i < n; ++i) { h ^= b[i]; h *= 0x100000001B3ull; }
    }
    template<class T> void num(T v) { const uint64_t x = static_cast<uint64_t>(v); bytes(&x, sizeof(x)); }
    template<class T> void vec(const std::vector<T>& v) { num(v.size()); if (!v.empty()) bytes(v.data(), v.size() * sizeof(T)); }
    void index(const HostIndex& X) {
        num(X.len); num(X.n_entries); num(X.nseg); num(X.wide); num(X.slot_mask);
        for (int c = 0; c < 4; ++c) num(X.nwalk[c]);
        for (int s = 0; s < SCG_MAX_SEGMENTS; ++s) num(X.segmask[s]);
        vec(X.nodes);
        vec(X.tables);
    }
};

// n distinct sequences (as far as 4^len allows) from raw generator outputs.
static std::vector<std::string> seeded_pool(uint64_t seed, int len, int n) {
    std::mt19937_64 rng(seed);
    std::set<std::string> seen;
    std::vector<std::string> pool;
    for (int tries = 0; static_cast<int>(pool.size()) < n && tries < 4 * n + 64; ++tries) {
        std::string s(static_cast<size_t>(len), 'A');
        for (auto& c : s) c = "ACGT"[rng() % 4];
        if (seen.insert(s).second) pool.push_back(s);
    }
    return pool;
}

static void digest_case(const char* name, const std::vector<std::string>& pool, int len, int mm, int cls) {
    std::vector<const char*> p;
    for (auto& s : pool) p.push_back(s.c_str());
    try {
        Fnv f;
        f.index(index_of(p, len, mm, cls));
        printf("%s index %016llx\n", name, static_cast<unsigned long long>(f.h));
    } catch (const Error& e) {
        printf("%s index error %d: %s\n", name, e.code, e.what());
    }
    try {
        Fnv f;
        Expansions exp;
        std::vector<uint64_t> uid_keys;
        f.index(uid_index_of(p, len, mm, cls, exp, uid_keys));
        f.num(exp.size());
        for (auto& x : exp) f.vec(x);
        f.vec(uid_keys);
        printf("%s uid %016llx\n", name, static_cast<unsigned long long>(f.h));
    } catch (const Error& e) {
        printf("%s uid error %d: %s\n", name, e.code, e.what());
    }
}

static int digests() {
    char name[96];
    uint64_t seed = 1000;
    auto random_case = [&](int len, int n, int mm, int cls) {
        snprintf(name, sizeof(name), "len%d_n%d_mm%d_class%d", len, n, mm, cls);
        digest_case(name, seeded_pool(++seed, len, n), len, mm, cls);
    };
    // short keys: budgets 2 and 3 leave position groups empty
    random_case(1, 3, 2, 0); random_case(1, 3, 3, 0); random_case(2, 10, 2, 0); random_case(2, 10, 3, 0); random_case(3, 40, 2, 0); random_case(3, 40, 3, 0);
    for (int mm = 0; mm <= 4; ++mm) {                                           // every budget in every class; 4: no tables
        random_case(20, 300, mm, 0); random_case(40, 300, mm, 1); random_case(100, 300, mm, 2);
    }
    random_case(32, 300, 1, 0); random_case(33, 300, 1, 1); random_case(64, 300, 2, 1); random_case(65, 300, 2, 2); random_case(256, 300, 3, 2);   // class edges
    random_case(20, 300, 1, 1); random_case(20, 300, 2, 2); random_case(40, 300, 3, 2);                               // a pool in a wider class than its own
    for (int cls = 0; cls < 3; ++cls) {                                                                              // no barcodes, one barcode
        random_case(0, 0, 1, cls);
        random_case(cls == 0 ? 20 : (cls == 1 ? 40 : 100), 0, 2, cls);
        random_case(cls == 0 ? 20 : (cls == 1 ? 40 : 100), 1, 3, cls);
    }
    random_case(20, 5000, 1, 0); random_case(20, 33000, 1, 0);                                                       // both steps of the slot count
    random_case(64, 5000, 2, 1); random_case(64, 33000, 2, 1); random_case(256, 5000, 3, 2); random_case(100, 33000, 1, 2);

    // the narrow key with every bit set (32 x G)
    {
        std::vector<std::string> pool = seeded_pool(++seed, 32, 300);
        pool[17] = std::string(32, 'G');
        digest_case("all_g", pool, 32, 1, 0);
        pool[5] = std::string(31, 'G') + "R";
        pool[17] = std::string(31, 'G') + "K";
        digest_case("all_g_twice", pool, 32, 2, 0);
    }
    // ambiguity codes, the duplicate error and the unknown base in every class
    for (int cls = 0; cls < 3; ++cls) {
        const int len = cls == 0 ? 20 : (cls == 1 ? 40 : 100);
        std::vector<std::string> pool = seeded_pool(++seed, len, 300);
        pool[3][len / 2] = 'N';
        pool[200][1] = 'R'; pool[200][len - 1] = 'Y';
        pool[299][0] = 'b';
        snprintf(name, sizeof(name), "iupac_class%d", cls);
        digest_case(name, pool, len, 1, cls);
        pool[250] = pool[40]; pool[250][7] = 'S';             // one of its two sequences is barcode 41's, or a neighbour's
        pool[40][7] = 'C';
        snprintf(name, sizeof(name), "shared_sequence_class%d", cls);
        digest_case(name, pool, len, 2, cls);
        pool[100][2] = 'Z';                                   // reported before the duplicates
        snprintf(name, sizeof(name), "unknown_base_class%d", cls);
        digest_case(name, pool, len, 2, cls);
    }
    // the length caps and the expansion limit
    digest_case("too_long_class0", seeded_pool(++seed, 33, 2), 33, 1, 0);
    {
        std::vector<std::string> pool = seeded_pool(++seed, 257, 2);
        pool[1][0] = 'Z';                                     // the cap comes first
        digest_case("too_long_class2", pool, 257, 1, 2);
    }
    digest_case("too_many_class0", std::vector<std::string>(2, std::string(13, 'N')), 13, 1, 0);
    digest_case("too_many_class1", std::vector<std::string>(1, std::string(40, 'N')), 40, 1, 1);
    return 0;
}

// ---- build times ----

static int times(int reps) {
    struct { const char* name; int len, n, mm, cls; bool uid; } cases[] = {
        {"narrow 100000 x 20, budget 1, index", 20, 100000, 1, 0, false}, {"wide 33000 x 64, budget 2, index", 64, 33000, 2, 1, false},
        {"big 5000 x 256, budget 3, index", 256, 5000, 3, 2, false}, {"narrow 100000 x 20, budget 1, uid index", 20, 100000, 1, 0, true}};
    for (auto& c : cases) {
        const std::vector<std::string> pool = seeded_pool(7, c.len, c.n);
        std::vector<const char*> p;
        for (auto& s : pool) p.push_back(s.c_str());
        double best = 1e30;
        for (int r = 0; r < reps; ++r) {
            const auto t0 = std::chrono::steady_clock::now();
            Expansions exp;
            std::vector<uint64_t> uid_keys;
            const HostIndex X = c.uid ? uid_index_of(p, c.len, c.mm, c.cls, exp, uid_keys) : index_of(p, c.len, c.mm, c.cls);
            const double ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
            if (static_cast<size_t>(X.n_entries) != pool.size()) return 1;
            best = std::min(best, ms);
        }
        printf("%-42s min of %d: %8.2f ms\n", c.name, reps, best);
    }
    return 0;
}

int main(int argc, char** argv) {
    if (argc > 1 && !strcmp(argv[1], "digest")) return digests();
    if (argc > 1 && !strcmp(argv[1], "time")) return times(argc > 2 ? atoi(argv[2]) : 10);
    const uint64_t seed = argc > 1 ? strtoull(argv[1], nullptr, 10) : 1;
    const int rounds = argc > 2 ? atoi(argv[2]) : 50;
    return random_rounds(seed, rounds, argc > 3 ? atoi(argv[3]) : rounds / 4);
}
