// scg_host.h -- internal C++ interface of the host runtime (not part of the C ABI).
#ifndef SCG_HOST_H
#define SCG_HOST_H

#include <cstdint>
#include <stdexcept>
#include <string>
#include <vector>

#include "../../include/scg.h"
#include "scg_common.h"

namespace scg {

// Carries an SCG_ERR_* code to the C boundary, where it becomes (code, message).
struct Error : std::runtime_error {
    int code;
    Error(int c, const std::string& msg) : std::runtime_error(msg), code(c) {}
};

// ---------------------------------------------------------------------------------------------
// Template: kaori/ScanTemplate.hpp:53-95.
// ---------------------------------------------------------------------------------------------
struct HostTemplate {
    ScgTemplate t;
    bool fwd, rev;
};
// strand: 0 forward, 1 reverse, 2 both.  Throws Error(SCG_ERR_INVALID) like the reference.
HostTemplate parse_template(const char* constant, int strand);

// ---------------------------------------------------------------------------------------------
// Pools: src/utils.cpp:5-23 (equal lengths), kaori/BarcodeSearch.hpp:23-60 (fill_library),
// kaori/MismatchTrie.hpp:93-205 (IUPAC expansion, DuplicateAction::ERROR).
// ---------------------------------------------------------------------------------------------
int pool_length(const char* const* pool, int32_t n);   // throws if lengths differ

// Key classes: 0 = up to 32 bases (2 x 32-bit planes), 1 = up to 64 ("wide"), 2 = up to 256 ("big"), the longest a template
// can be (src/count_single_barcodes.cpp:37-47).  Pools that meet in one kernel (both regions of a combination, both mates
// of a pair) are built in the widest class among them; concatenated multi-region keys are never narrow.
inline int key_class(int len) { return len > SCG_MAX_WIDE_BARCODE ? 2 : (len > SCG_MAX_BARCODE ? 1 : 0); }

// A node or slot is {key lo, key hi, value, next} in class 0, {lo64, hi64, value, next, 0, 0} in class 1 and
// {lo x 4, hi x 4, value, next, 0, 0} (as 64-bit words) in class 2: 4, 8 and 20 32-bit words (ScgIndex).
struct HostIndex {
    int32_t len = 0;
    int32_t n_entries = 0;
    int32_t nseg = 0;
    int wide = 0;                    // the key class (ScgIndex::wide)
    uint32_t slot_mask = 0;
    int32_t nwalk[4] = {0, 0, 0, 0};
    uint64_t segmask[SCG_MAX_SEGMENTS] = {0, 0, 0, 0, 0, 0};
    std::vector<uint32_t> nodes;     // [max(nseg,1)][n_entries] nodes, `next` being the next entry in table s's chain
    std::vector<uint32_t> tables;    // [nseg][slot_mask + 1] slots: head node of the chain keyed in that slot
};

// The index of a pool of `len` bases in key class `cls` >= key_class(len).  max_mm is the plan's mismatch budget for this
// pool: the index gets max_mm + 1 segments (none, i.e. dense scans, when that exceeds SCG_MAX_SEGMENTS).
// value = barcode index; two barcodes sharing one concrete sequence => Error("duplicate sequences
// detected (a, b) when constructing the trie").
HostIndex build_index(const char* const* pool, int32_t n, int32_t len, int max_mm, int cls);

// value = uid of the concrete sequence (duplicates within the pool merge; n_entries is the number of uids).
// expansions[i] receives the uids of barcode i's concrete expansions, in lexicographic (A,C,G,T) order; uid_keys the key of
// every uid in class 0 (for the pair table's dense list), nothing in the others.
HostIndex build_uid_index(const char* const* pool, int32_t n, int32_t len, int max_mm, int cls,
                          std::vector<std::vector<int32_t> >& expansions, std::vector<uint64_t>& uid_keys);

struct HostPairTable {
    int32_t n_entries = 0;
    uint32_t mask = 0;
    std::vector<uint64_t> keys;
    std::vector<int32_t> vals;
    std::vector<uint64_t> list_key1, list_key2;
    std::vector<int32_t> list_vals;
};
HostPairTable build_pair_table(const std::vector<std::vector<int32_t> >& exp1, const std::vector<uint64_t>& uid_keys1,
                               const std::vector<std::vector<int32_t> >& exp2, const std::vector<uint64_t>& uid_keys2);

// The staged-scan description of a template for a mismatch budget: bit planes of the constant
// bases and the pigeonhole seeds of both strands.
ScgScan build_scan(const ScgTemplate& t, int max_mm);


// ---------------------------------------------------------------------------------------------
// FASTQ: kaori/FastqReader.hpp:42-110 over byteme readers.
// ---------------------------------------------------------------------------------------------
struct ReadBatch {
    std::vector<char> seqs;
    std::vector<uint64_t> offsets;   // n + 1
    int64_t size() const { return static_cast<int64_t>(offsets.size()) - 1; }
    void clear() { seqs.clear(); offsets.assign(1, 0); }
};

class FastqStream {
public:
    explicit FastqStream(const char* path);
    ~FastqStream();
    FastqStream(const FastqStream&) = delete;
    FastqStream& operator=(const FastqStream&) = delete;

    // Appends up to max_reads records / max_bytes sequence bytes to `out` (which is cleared first).
    // Returns false once the file is exhausted and nothing was appended.
    bool next_batch(ReadBatch& out, int64_t max_reads, int64_t max_bytes);

private:
    struct Impl;
    Impl* impl;
};

// ---------------------------------------------------------------------------------------------
// Parallel staging of plain (uncompressed) FASTQ files made of ordinary 4-line records.
//
// The file is mapped and cut into windows; inside a window every worker thread starts at a
// position that *looks like* a record start and parses strict 4-line records up to the next
// worker's start.  A worker's start is only trusted once its predecessor has landed on it exactly,
// and the first worker starts on a verified boundary, so by induction the result equals the
// sequential reference parse (kaori/FastqReader.hpp:42-110) whenever every record satisfies:
// '@' first, no '+' inside the sequence line, '+' line third, quality as long as the sequence.
// Anything else (multi-line records, malformed input, a missed landing) makes `unusual()` return
// true, and the caller redoes the file with the sequential FastqStream, which reproduces the
// reference's behaviour and error messages exactly.
// ---------------------------------------------------------------------------------------------
class ParallelFastq {
public:
    // Throws Error(SCG_ERR_IO) if the file cannot be opened / mapped.
    ParallelFastq(const char* path, int nthreads);
    ~ParallelFastq();
    ParallelFastq(const ParallelFastq&) = delete;
    ParallelFastq& operator=(const ParallelFastq&) = delete;

    static bool is_plain_file(const char* path);   // exists, regular, not gzip

    // Parses the next window into one batch per worker (empty batches possible).
    // Returns false when the file is exhausted or the input turned out to be unusual.
    bool next_window(std::vector<ReadBatch>& out);
    bool unusual() const;

private:
    struct Impl;
    Impl* impl;
};

int default_host_threads(int requested, int devices = 1);

} // namespace scg

#endif
