// scg_launch.h -- launchers exported by scg_kernels.hip to the host runtime.
#ifndef SCG_LAUNCH_H
#define SCG_LAUNCH_H

#include <hip/hip_runtime_api.h>

#include "../../include/scg.h"
#include "scg_common.h"

namespace scg {

// Whether the staged kernels take a batch whose longest read has max_len bases (0: unknown); the byte-wise general
// kernels take the rest.  Test hook: SCG_FORCE_GENERAL=1 (any value but empty / 0) gives them every batch; read at
// every launch.
bool staged_takes(int max_len);

hipError_t launch_single(const ScgSingleParams& P, int tmpl_len, const ScgReads& R, int64_t n, const ScgCounters& counts, int32_t* flag, hipStream_t stream);
// kaori::SimpleSingleMatch::State of every read (scg_assign_batch): launch_single's dispatch, no counters touched
hipError_t launch_assign(const ScgSingleParams& P, int tmpl_len, const ScgReads& R, int64_t n, const ScgAssignOut& out, int32_t* flag, hipStream_t stream);
// kaori::SingleBarcodePairedEnd: the barcode of pair i is looked for on read i of R1 and of R2
hipError_t launch_single_paired(const ScgSingleParams& P, int tmpl_len, const ScgReads& R1, const ScgReads& R2, int64_t n, const ScgCounters& counts, int32_t* flag,
                                hipStream_t stream);
// countRandomBarcodes: d_hits[i] = (position << 1) | reverse of read i's template hit, or -1
hipError_t launch_random(const ScgSingleParams& P, int tmpl_len, const ScgReads& R, int64_t n, int32_t* d_hits, int32_t* flag, hipStream_t stream);
hipError_t launch_combo(const ScgComboParams& P, int tmpl_len, const ScgReads& R, int64_t n, const ScgCounters& cells, int32_t* flag, hipStream_t stream);
// combinations over P.nreg variable regions: cell / key of read i = its mixed-radix key (ScgComboRegionsParams); `cells` counts
// with atomics or carries a key stream (unit_pair), no index stream
hipError_t launch_combo_regions(const ScgComboRegionsParams& P, int tmpl_len, const ScgReads& R, int64_t n, const ScgCounters& cells, int32_t* flag, hipStream_t stream);
hipError_t launch_dual(const ScgDualParams& P, int tmpl_len, const ScgReads& R1, const ScgReads& R2, int64_t n, const ScgCounters& counts, int32_t* flag, hipStream_t stream);
hipError_t launch_fold(int32_t* replicas, int replica_shift, int64_t n, int32_t* counters, hipStream_t stream);
// hot[2][SCG_HOT_SLOTS] -> pair_of_counters[0], [1] (and clears the slots); ScgCounters::hot
hipError_t launch_hot_fold(int32_t* hot, int32_t* pair_of_counters, hipStream_t stream);
// counters[unit_index[r]] += 1 for every r with unit_index[r] >= 0, through LDS histograms (ScgCounters::unit_index)
hipError_t launch_tally(const int32_t* unit_index, int64_t n, int32_t* counters, int64_t n_counters, hipStream_t stream);
// Combination streams (ScgCounters::unit_pair) -> runs of (distinct key, count): scg_sparse.hip.  d_sorted, d_unique: n keys
// each; d_counts: n; d_runs: 1; scratch of sort_rle_scratch_bytes(n).
size_t sort_rle_scratch_bytes(size_t n);
hipError_t launch_sort_rle(const uint64_t* d_keys, uint64_t* d_sorted, size_t n, uint64_t* d_unique, uint32_t* d_counts, uint32_t* d_runs,
                           void* d_scratch, size_t scratch_bytes, hipStream_t stream);
// ---- combination counts of many files as one matrix (scg_combine.hip) ----
// Dense cells -> (key, count) pairs of the non-zero cells, in cell order = ascending key order (key = first << 32 | second,
// cell = first * n1 + second).  One tile of SCG_COMPACT_TILE_CELLS cells per 256-lane workgroup, two passes with a scan of
// the tiles' counts between them; no atomics, no workgroup waits for another.
#define SCG_COMPACT_TILE_CELLS 4096
inline uint64_t compact_tiles(uint64_t n_cells) { return (n_cells + SCG_COMPACT_TILE_CELLS - 1) / SCG_COMPACT_TILE_CELLS; }
size_t compact_scan_scratch_bytes(uint64_t n_cells);
// Pass 1 and the scan: d_tile_offsets[t] = non-zero cells in the tiles before t, for t = 0 .. compact_tiles(n_cells); the
// last entry is their number K.  d_tile_offsets and d_tile_counts: compact_tiles(n_cells) + 1 entries each.  cells must be
// 16-byte aligned.
hipError_t launch_compact_count(const int32_t* cells, uint64_t n_cells, unsigned long long* d_tile_counts, unsigned long long* d_tile_offsets,
                                void* d_scratch, size_t scratch_bytes, hipStream_t stream);
// Pass 2 over the same, unchanged cells: keys_out / counts_out get the K pairs.
hipError_t launch_compact_scatter(const int32_t* cells, uint64_t n_cells, uint32_t n1, const unsigned long long* d_tile_offsets,
                                  uint64_t* keys_out, int32_t* counts_out, hipStream_t stream);
// Rows of a union: rows_out[i] = the place of keys[i] in the ascending distinct keys d_unique[0 .. *d_n_unique), for n
// entries; *d_flag is set when a key is not among them (never expected).
hipError_t launch_union_rows(const uint64_t* keys, uint64_t n, const uint64_t* d_unique, const uint32_t* d_n_unique, int32_t* rows_out,
                             int32_t* d_flag, hipStream_t stream);
// One file's list, sorted by key: keys and their counts (n entries, 64 key bits); scratch of sort_pairs_scratch_bytes(n).
size_t sort_pairs_scratch_bytes(size_t n);
hipError_t launch_sort_pairs(const uint64_t* keys_in, uint64_t* keys_out, const int32_t* vals_in, int32_t* vals_out, size_t n,
                             void* d_scratch, size_t scratch_bytes, hipStream_t stream);
// *d_flag is set when two neighbours of the sorted list keys[0 .. n) are equal.
hipError_t launch_flag_equal_neighbours(const uint64_t* keys, uint64_t n, int32_t* d_flag, hipStream_t stream);

// ---- random-barcode plans: the tally in HBM (scg_random.hip) ----
// Open-addressing table of capacity mask + 1 (a power of two).  Slot s: tags[s] (0 = empty), counts[s], and for hashed
// tags the key bytes at arena[s * vlen].  Tag layout: bit 63 clear, bit 62 set, 2 bits per base MSB first below = a
// packed key of pure upper-case ACGT of at most 31 bases; bit 63 set = a hashed key, bits 61-62 the round, the hash of
// the bytes below (kept to tag_bits bits).  state[0]: the first unknown-base error, (read ordinal << 8) | byte, ~0 if
// none; state[1]: occupied slots; state[2]: reads whose key collided in every round.
// Files mode (scg_count_random_barcodes_files; `ids` non-null): slot s also carries ids[s], the value of state[1] when
// the slot was claimed -- a row number that stays with the key through every rehash and soft reset.
#define SCG_RANDOM_ROUNDS 4
struct ScgRandomTable {
    unsigned long long* tags;
    unsigned long long* counts;
    uint8_t* arena;
    uint32_t* ids;             // null: plans of scg_plan_random keep no ids
    unsigned long long* state;
    uint64_t mask;
    int32_t vstart, vlen;      // the first forward variable region (the key on both strands)
    int32_t tag_bits;          // hash bits kept in a hashed tag (61; fewer only under the test hook)
    int32_t pad;
};
// Round 0 of a batch: the key of every hit, aggregated per workgroup in LDS, claimed or found in the table;
// slots[i] = its slot (bit 30 set for a hashed key; capacity <= 2^30) or -1.  ordinal0: counting-order number of read 0 (for the unknown-base error).
hipError_t launch_random_insert(const ScgRandomTable& T, const ScgReads& R, int64_t n, const int32_t* hits, int32_t* slots,
                                int64_t ordinal0, hipStream_t stream);
// Round 0's verify: reads whose hashed key differs from its slot's arena bytes give back their count and join list_out
// (lens[1] entries).  Then rounds 1 .. SCG_RANDOM_ROUNDS - 1 over the lists, lengths read on the device (lens[r]).
// list_a, list_b: n entries each; lens: SCG_RANDOM_ROUNDS int32, zero on entry.
hipError_t launch_random_verify_rounds(const ScgRandomTable& T, const ScgReads& R, int64_t n, const int32_t* hits, int32_t* slots,
                                       int32_t* list_a, int32_t* list_b, int32_t* lens, hipStream_t stream);
// Moves every entry of `from` into `to` (empty, larger), ids included; tags are capacity-independent and distinct.
hipError_t launch_random_rehash(const ScgRandomTable& from, const ScgRandomTable& to, hipStream_t stream);
// Files mode, behind a file's last batch: every slot with a count appends (id, count) to `list` (pairs of int32, room for
// list_cap of them) and its count is cleared; tag, key and id stay.  n_out[0]: pairs appended; n_out[1]: non-zero when a
// count exceeds INT32_MAX or the list is too short (both zero on entry).  Nothing else may touch the table meanwhile.
hipError_t launch_random_harvest(const ScgRandomTable& T, int32_t* list, uint32_t list_cap, unsigned int* n_out, hipStream_t stream);
// Read-out: occupied slots with a count -> packed (tag, count) and hashed (slot, count) lists; n_out[0] / n_out[1]
// their lengths (zero on entry); each list has room for every occupied slot.  with_ids: EVERY occupied slot, and its id
// in the place of its count (the keys of a files-mode table, whose counts the harvests have taken).
hipError_t launch_random_compact(const ScgRandomTable& T, unsigned long long* packed_tags, unsigned long long* packed_counts,
                                 int32_t* hashed_slots, unsigned long long* hashed_counts, unsigned long long* n_out, bool with_ids,
                                 hipStream_t stream);
size_t random_sort_scratch_bytes(size_t n);
// Packed tags sorted with their counts on bits [0, end_bit): numeric order of packed tags is byte-wise order of the keys.
hipError_t launch_random_sort(const unsigned long long* keys_in, unsigned long long* keys_out, const unsigned long long* vals_in,
                              unsigned long long* vals_out, size_t n, int end_bit, void* scratch, size_t scratch_bytes, hipStream_t stream);
// Packed tags -> n rows of vlen characters and a NUL (stride vlen + 1).
hipError_t launch_random_decode(const unsigned long long* tags, int64_t n, int32_t vlen, char* out, hipStream_t stream);
// Arena bytes of n slots -> n rows of vlen bytes.
hipError_t launch_random_gather(const ScgRandomTable& T, const int32_t* slots, int64_t n, uint8_t* out, hipStream_t stream);

hipError_t launch_match(const ScgIndex& tab, const uint8_t* d_seqs, int32_t n, int cap, int reverse,
                        int32_t* d_index, int32_t* d_mm, hipStream_t stream);
hipError_t launch_synth(const scg_synth_spec& S, char* d_out, int64_t n, hipStream_t stream);

} // namespace scg

#endif
