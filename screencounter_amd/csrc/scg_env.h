// scg_env.h -- every SCG_* environment switch of the library, read in one place (DESIGN.md §5 has the table).
//
// The rule: the environment is read on the calling thread when a call enters the library and no other call is in
// flight.  Everything that call does, on whatever thread, sees that one snapshot.
//
// A call enters through guarded() (scg_internal.hpp), which opens an EnvScope; the scope that finds no other open takes
// the snapshot, nested and overlapping ones leave it alone.  Every thread the library starts is joined, or idle on a
// condition variable, before the call that started it returns, so none reads env() between calls.  A program that never
// opens a scope (the stand-alone test drivers call internal functions directly) gets the snapshot at its first env().
// Plain host C++, nothing from HIP, header-only.
#ifndef SCG_ENV_H
#define SCG_ENV_H

#include <algorithm>
#include <atomic>
#include <cstddef>
#include <cstdint>
#include <cstdlib>
#include <mutex>
#include <string>
#include <type_traits>

namespace scg {

// One field per switch, holding the built-in default.  Classes: a SETTING is the user's to choose (devices, threads); a
// TUNING AID moves a threshold or picks a variant for measurements; a TEST HOOK forces a path or a tiny size so that
// tests reach it.  Tuning aids and test hooks never change counts.
struct Env {
    static constexpr int SEED_LEN = 10;         // == SCG_SEED_LEN of scg_common.h, which needs HIP (scg_library.cpp asserts it)

    bool device_set = false; int device = -1;   // SCG_DEVICE: the device of plans and of the calling thread's files when non-empty (setting)
    bool devices_set = false; std::string devices;   // SCG_DEVICES: "all" or a comma list, parsed by device_list(); set = non-empty (setting)
    int host_threads = 0;                       // SCG_HOST_THREADS >= 1: host threads of a file-level call; 0 = by CPUs and devices (setting)

    int replica_addr_log2 = 20;                 // SCG_REPLICA_ADDR_LOG2: counter replicas spread the atomics over 2^this addresses (tuning aid)
    int64_t dense_cells = int64_t(1) << 26;     // SCG_DENSE_CELLS in [0, 2^30]: combination spaces beyond it take sparse mode (tuning aid)
    int tally = -1;                             // SCG_TALLY: 0 / 1 forces tally mode off / on; -1 = by library and batch size (tuning aid)
    size_t extra_lds_kb = 0;                    // SCG_EXTRA_LDS_KB: unused dynamic LDS per workgroup of the staged kernels (tuning aid)
    int dual_two_tiles = -1;                    // SCG_DUAL_TWO_TILES: 1 / 0 forces the two-tile / the passes pair search; -1 = by template (tuning aid)
    bool inflate_lanes = true;                  // SCG_INFLATE_LANES=0: the BGZF decoder that walks every symbol with the whole wavefront (tuning aid)
    int table_factor = 0;                       // SCG_TABLE_FACTOR >= 2: slots per entry of the index tables; 0 = by library size (tuning aid)
    int seed_max = SEED_LEN - 1;                // SCG_SEED_MAX in [4, SEED_LEN]: most constant bases a seed takes (tuning aid)
    double gzip_whole_gb = 8.0;                 // SCG_GZIP_WHOLE_GB >= 0: largest text libdeflate inflates whole; 0 = never (tuning aid)
    bool libdeflate = true;                     // SCG_LIBDEFLATE=0: zlib alone (tuning aid)
    bool trace = false;                         // SCG_TRACE=1: stage timings and the rungs taken, on stderr (tuning aid)

    bool force_general = false;                 // SCG_FORCE_GENERAL=1: the byte-wise general kernels alone (test hook)
    bool device_scan = true;                    // SCG_DEVICE_SCAN=0: the host readers parse the records (test hook)
    bool host_scan = true;                      // SCG_HOST_SCAN=0: plain files ship their raw text too (test hook)
    bool buffer_cache = true;                   // SCG_BUFFER_CACHE=0: no idle scan slots or gunzip scratch kept for the next call (test hook)
    bool device_inflate = true, inflate_strict = false;   // SCG_DEVICE_INFLATE=0: BGZF members inflate on the host; =2: a hand-back is an error (test hook)
    bool device_gunzip = true, gunzip_strict = false;     // SCG_DEVICE_GUNZIP=0: no gzip decoding on the device; =2: a hand-back is an error (test hook)
    bool pgzip = true;                          // SCG_PGZIP=0: single inflate streams instead of the parallel gzip decoder (test hook)
    size_t window_kb = 0;                       // SCG_WINDOW_KB: text window size; 0 = the built-in sizes (test hook)
    size_t fastq_piece_kb = size_t(32) << 10;   // SCG_FASTQ_PIECE_KB > 0: text per host thread and window of the parallel parser (test hook)
    int random_tag_bits = 61;                   // SCG_TEST_RANDOM_TAG_BITS in [0, 61]: hash bits a random-barcode tag keeps (test hook)
    bool dgzip_tiny = false; size_t dgzip_chunk_kb = 64;   // SCG_DGZIP_CHUNK_KB >= 4: device gunzip chunk; set at all = files from 64 bytes, not 2 MB (test hook)
    uint32_t dgzip_tail_group = 32;             // SCG_DGZIP_TAIL_GROUP >= 1: chunks per group of the tails' scan (test hook)
    uint64_t dgzip_min_member_chunks = 32;      // SCG_DGZIP_MIN_MEMBER_CHUNKS >= 0: smallest inner member the device decodes (test hook)
    uint64_t dgzip_group_kb = uint64_t(512) << 10;   // SCG_DGZIP_GROUP_KB >= 4: compressed bytes decoded per group (test hook)
    size_t pgzip_chunk_kb = 0;                  // SCG_PGZIP_CHUNK_KB >= 1: parallel gzip chunk; 0 = by file size and threads (test hook)
    size_t pgzip_cap_kb = 0;                    // SCG_PGZIP_CAP_KB >= 1: symbols (in 1024s) a chunk may decode to; 0 = by chunk size (test hook)
#ifdef SCG_ABLATE
    int ablate = 0;                             // SCG_ABLATE: phase-ablation mask of the measurement builds (tuning aid; not in the product library)
#endif

    // The only getenv of the library.  Each switch keeps the parsing rule it always had, oddities included.
    static Env read() {
        auto raw = [](const char* name) { return std::getenv(name); };
        auto first = [](const char* name) { const char* e = std::getenv(name); return e ? *e : '\0'; };
        auto flag = [](const char* name) { const char* e = std::getenv(name); return e && *e && *e != '0'; };
        auto filled = [](const char* name) { const char* e = std::getenv(name); return e && *e ? e : nullptr; };   // set and not empty
        auto at_least = [](auto v, auto lo, auto& field) { if (v >= lo) field = static_cast<std::decay_t<decltype(field)>>(v); };   // else: the default
        Env x;
        if (const char* e = filled("SCG_DEVICE")) { x.device_set = true; x.device = std::atoi(e); }
        if (const char* e = filled("SCG_DEVICES")) { x.devices_set = true; x.devices = e; }
        if (const char* e = raw("SCG_HOST_THREADS")) at_least(std::atoi(e), 1, x.host_threads);
        if (const char* e = raw("SCG_REPLICA_ADDR_LOG2")) x.replica_addr_log2 = std::atoi(e);
        if (const char* e = filled("SCG_DENSE_CELLS")) x.dense_cells = std::min<int64_t>(std::max<int64_t>(std::atoll(e), 0), int64_t(1) << 30);
        if (const char* e = filled("SCG_TALLY")) x.tally = *e != '0';
        if (const char* e = raw("SCG_EXTRA_LDS_KB")) x.extra_lds_kb = static_cast<size_t>(std::atoi(e));
        if (const char* e = filled("SCG_DUAL_TWO_TILES")) x.dual_two_tiles = std::atoi(e);
        x.inflate_lanes = first("SCG_INFLATE_LANES") != '0';
        if (const char* e = raw("SCG_TABLE_FACTOR")) at_least(std::atoi(e), 2, x.table_factor);
        if (const char* e = raw("SCG_SEED_MAX")) { const int v = std::atoi(e); if (v >= 4 && v <= SEED_LEN) x.seed_max = v; }
        if (const char* e = raw("SCG_GZIP_WHOLE_GB")) x.gzip_whole_gb = std::max(0.0, std::atof(e));
        x.libdeflate = first("SCG_LIBDEFLATE") != '0';
        x.trace = flag("SCG_TRACE");
        x.force_general = flag("SCG_FORCE_GENERAL");
        x.device_scan = first("SCG_DEVICE_SCAN") != '0';
        x.host_scan = first("SCG_HOST_SCAN") != '0';
        x.buffer_cache = first("SCG_BUFFER_CACHE") != '0';
        x.device_inflate = first("SCG_DEVICE_INFLATE") != '0';
        x.inflate_strict = first("SCG_DEVICE_INFLATE") == '2';
        x.device_gunzip = first("SCG_DEVICE_GUNZIP") != '0';
        x.gunzip_strict = first("SCG_DEVICE_GUNZIP") == '2';
        x.pgzip = first("SCG_PGZIP") != '0';
        if (const char* e = raw("SCG_WINDOW_KB")) x.window_kb = static_cast<size_t>(std::max(0L, std::atol(e)));
        if (const char* e = raw("SCG_FASTQ_PIECE_KB")) at_least(std::atol(e), 1L, x.fastq_piece_kb);
        if (const char* e = filled("SCG_TEST_RANDOM_TAG_BITS")) x.random_tag_bits = std::min(std::max(std::atoi(e), 0), 61);
        if (const char* e = raw("SCG_DGZIP_CHUNK_KB")) { x.dgzip_tiny = true; at_least(std::atol(e), 4L, x.dgzip_chunk_kb); }
        if (const char* e = raw("SCG_DGZIP_TAIL_GROUP")) x.dgzip_tail_group = static_cast<uint32_t>(std::max(1L, std::atol(e)));
        if (const char* e = raw("SCG_DGZIP_MIN_MEMBER_CHUNKS")) x.dgzip_min_member_chunks = static_cast<uint64_t>(std::max(0L, std::atol(e)));
        if (const char* e = raw("SCG_DGZIP_GROUP_KB")) at_least(std::atol(e), 4L, x.dgzip_group_kb);
        if (const char* e = raw("SCG_PGZIP_CHUNK_KB")) at_least(std::atol(e), 1L, x.pgzip_chunk_kb);
        if (const char* e = raw("SCG_PGZIP_CAP_KB")) at_least(std::atol(e), 1L, x.pgzip_cap_kb);
#ifdef SCG_ABLATE
        if (const char* e = raw("SCG_ABLATE")) x.ablate = std::atoi(e);
#endif
        return x;
    }
};

namespace envdetail {
inline std::mutex mu;
inline int in_flight = 0;                       // open scopes (under mu)
inline std::atomic<bool> taken{false};          // the snapshot exists
inline Env snapshot;
}

// A call's stay in the library.  The scope that takes the count of open scopes from 0 to 1 reads the environment.
struct EnvScope {
    EnvScope() {
        std::lock_guard<std::mutex> g(envdetail::mu);
        if (envdetail::in_flight++ == 0) {
            envdetail::snapshot = Env::read();
            envdetail::taken.store(true, std::memory_order_release);
        }
    }
    ~EnvScope() {
        std::lock_guard<std::mutex> g(envdetail::mu);
        --envdetail::in_flight;
    }
    EnvScope(const EnvScope&) = delete;
    EnvScope& operator=(const EnvScope&) = delete;
};

// The snapshot.  No lock once it exists; without any scope so far, the first use takes it.
inline const Env& env() {
    if (!envdetail::taken.load(std::memory_order_acquire)) {
        std::lock_guard<std::mutex> g(envdetail::mu);
        if (!envdetail::taken.load(std::memory_order_relaxed)) {
            envdetail::snapshot = Env::read();
            envdetail::taken.store(true, std::memory_order_release);
        }
    }
    return envdetail::snapshot;
}

}  // namespace scg

#endif
