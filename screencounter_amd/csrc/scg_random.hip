// scg_random.hip -- countRandomBarcodes on reads resident in HBM: the tally of unknown keys as an open-addressing table in
// HBM.
//
// The template search is the existing random_staged_kernel / random_kernel (launch_random); these kernels take its hits:
//   insert   the key of every hit (raw bytes forward, complement_base<true> reverse complement on the reverse strand),
//            aggregated per workgroup in LDS, then one 64-bit CAS claims or finds the slot of each distinct tag and one
//            atomic add carries the workgroup's count.  The claimer stores the key bytes in the arena; nobody reads them
//            in this launch.
//   verify   (next launch, hashed keys only) every read compares its key with its slot's arena bytes; a read whose key
//            differs met a 64-bit tag collision: it takes its count back and joins the list of the next round, whose
//            hash seed differs.  The rounds read their list length on the device and exit at once when it is 0.
// Between workgroups of one launch only atomics pass information (the CAS result, the adds): no plain-stored byte is
// handed off inside a launch, so neither the per-CU L1 nor the per-XCD L2s can serve a stale copy; every plain-stored
// byte (arena, ids, lists, slots) is read in a later launch on the same stream.
//
// Files mode (scg_count_random_barcodes_files) keeps one table for all the files a device takes: the claimer of a slot
// also stores a row id there (the occupancy counter's value), the harvest kernel takes a file's (id, count) pairs out and
// clears the counts, and the keys leave the device once, at the end of the call, with their ids.
#include <cstring>

#include <hip/hip_runtime.h>
#include <rocprim/rocprim.hpp>

#include "scg_launch.h"

namespace scg {
namespace {

constexpr int RB = 256;                 // reads per workgroup
constexpr int WAVE = 64;                // lanes of a gfx950 wavefront (RB is a multiple)
constexpr int LDS_SLOTS = 2 * RB;       // LDS aggregation table: at most RB distinct tags, load <= 1/2
constexpr int ROUND_GRID = 256;         // workgroups of the list rounds (grid-stride over a length known on the device)
constexpr unsigned long long HASHED = 1ull << 63;
constexpr unsigned long long PACKED = 1ull << 62;
constexpr int32_t HASHED_SLOT = 1 << 30;   // slots[i]: slot index, this bit set when the key is hashed

__device__ __forceinline__ unsigned long long fmix64(unsigned long long x) {
    x ^= x >> 33; x *= 0xff51afd7ed558ccdull;
    x ^= x >> 33; x *= 0xc4ceb9fe1a85ec53ull;
    x ^= x >> 33;
    return x;
}

// complement_base<true> (kaori/utils.hpp): ACGTN in either case -> upper-case complement; -1 for any other byte
__device__ __forceinline__ int complement(int b) {
    switch (b) {
        case 'A': case 'a': return 'T';
        case 'C': case 'c': return 'G';
        case 'G': case 'g': return 'C';
        case 'T': case 't': return 'A';
        case 'N': case 'n': return 'N';
        default: return -1;
    }
}

// Byte j of the key whose region starts at p: the raw byte forward, the complement of byte vlen-1-j in reverse.
__device__ __forceinline__ int key_byte(const uint8_t* p, int j, int vlen, bool rev) {
    return rev ? complement(p[vlen - 1 - j]) : p[j];
}

// Where read i's key lies; false without a hit.  The window lies inside the read by construction of the hit; the
// bound is checked again so that no hit can send a load past its read.
__device__ __forceinline__ bool locate(const ScgRandomTable& T, const ScgReads& R, const int32_t* hits, int64_t i,
                                       const uint8_t*& p, bool& rev) {
    const int32_t h = hits[i];
    if (h < 0) return false;
    const uint8_t* base;
    int64_t n;
    if (R.offsets) {
        const uint32_t a = R.offsets[i], b = R.offsets[i + 1];
        base = R.seqs + a;
        n = (int64_t)b - (int64_t)a;
    } else {
        base = R.seqs + (size_t)i * (size_t)R.fixed_len;
        n = R.fixed_len;
    }
    const int64_t pos = (int64_t)(h >> 1) + T.vstart;
    if (pos + T.vlen > n) return false;
    p = base + pos;
    rev = (h & 1) != 0;
    return true;
}

// The key's tag in `round`, or 0 when the reverse complement meets an unknown base (*bad = that byte: the first one in
// key order, i.e. the rightmost of the region in the read, where the reference's loop throws).
__device__ __forceinline__ unsigned long long key_tag(const ScgRandomTable& T, const uint8_t* p, bool rev, int round, int* bad) {
    const int vlen = T.vlen;
    bool packable = vlen <= 31;
    unsigned long long packed = 0, w = 0;
    unsigned long long h = fmix64(0x9E3779B97F4A7C15ull * (unsigned long long)(round + 1) + (unsigned long long)vlen);
    for (int j = 0; j < vlen; ++j) {
        const int b = key_byte(p, j, vlen, rev);
        if (b < 0) { *bad = p[vlen - 1 - j]; return 0; }
        const int c = b == 'A' ? 0 : b == 'C' ? 1 : b == 'G' ? 2 : b == 'T' ? 3 : 4;
        packable = packable && c < 4;
        packed = (packed << 2) | (unsigned long long)(c & 3);
        w |= (unsigned long long)b << (8 * (j & 7));
        if ((j & 7) == 7) { h = fmix64(h ^ w) + 0x632BE59BD9B4E019ull; w = 0; }
    }
    if (packable && round == 0) return PACKED | packed;
    if (vlen & 7) h = fmix64(h ^ w);
    const unsigned long long keep = T.tag_bits >= 61 ? (1ull << 61) - 1 : (1ull << T.tag_bits) - 1;
    return HASHED | ((unsigned long long)round << 61) | (h & keep);
}

__device__ __forceinline__ bool same_key(const ScgRandomTable& T, uint64_t s, const uint8_t* p, bool rev) {
    const uint8_t* a = T.arena + s * (uint64_t)T.vlen;
    for (int j = 0; j < T.vlen; ++j) {
        if (key_byte(p, j, T.vlen, rev) != a[j]) return false;
    }
    return true;
}

__device__ __forceinline__ void store_key(const ScgRandomTable& T, uint64_t s, const uint8_t* p, bool rev) {
    uint8_t* a = T.arena + s * (uint64_t)T.vlen;
    for (int j = 0; j < T.vlen; ++j) a[j] = (uint8_t)key_byte(p, j, T.vlen, rev);
}

// Claims or finds the slot of `tag` (linear probing, one CAS per probe: the only look at a tag another workgroup may
// have written in this launch is the CAS's own result) and adds cnt.  -1 when no slot is free, which the host's growth
// rule (occupancy <= capacity / 2) excludes.
__device__ __forceinline__ int64_t table_insert(const ScgRandomTable& T, unsigned long long tag, unsigned long long cnt, bool& claimed) {
    uint64_t s = fmix64(tag) & T.mask;
    for (uint64_t probe = 0; probe <= T.mask; ++probe) {
        const unsigned long long old = atomicCAS(&T.tags[s], 0ull, tag);
        if (old == 0 || old == tag) {
            claimed = old == 0;
            atomicAdd(&T.counts[s], cnt);
            if (claimed) {
                const unsigned long long id = atomicAdd(&T.state[1], 1ull);
                if (T.ids) T.ids[s] = (uint32_t)id;              // (like the arena bytes: read by later launches only)
            }
            return (int64_t)s;
        }
        s = (s + 1) & T.mask;
    }
    claimed = false;
    return -1;
}

__global__ __launch_bounds__(RB) void random_insert_kernel(ScgRandomTable T, ScgReads R, int64_t n, const int32_t* __restrict__ hits,
                                                           int32_t* __restrict__ slots, int64_t ordinal0) {
    __shared__ unsigned long long ltag[LDS_SLOTS];
    __shared__ unsigned int lcount[LDS_SLOTS];
    __shared__ int32_t lslot[LDS_SLOTS];
    for (int k = threadIdx.x; k < LDS_SLOTS; k += RB) { ltag[k] = 0; lcount[k] = 0; }
    __syncthreads();
    const int64_t i = (int64_t)blockIdx.x * RB + threadIdx.x;
    const uint8_t* p = nullptr;
    bool rev = false, leader = false;
    int e = -1;
    unsigned long long tag = 0;
    if (i < n && locate(T, R, hits, i, p, rev)) {
        int bad = 0;
        tag = key_tag(T, p, rev, 0, &bad);
        if (!tag) {
            atomicMin(&T.state[0], ((unsigned long long)(ordinal0 + i) << 8) | (unsigned long long)(bad & 0xFF));
        } else {
            int k = (int)(fmix64(tag) & (LDS_SLOTS - 1));
            for (;;) {
                const unsigned long long old = atomicCAS(&ltag[k], 0ull, tag);
                if (old == 0) { leader = true; break; }
                if (old == tag) break;
                k = (k + 1) & (LDS_SLOTS - 1);
            }
            e = k;
            atomicAdd(&lcount[k], 1u);
        }
    }
    __syncthreads();
    if (leader) {
        bool claimed = false;
        const unsigned int c = lcount[e];
        const int64_t s = table_insert(T, tag, c, claimed);
        if (s < 0) {
            atomicAdd(&T.state[2], (unsigned long long)c);
            lslot[e] = -1;
        } else {
            if (claimed && (tag & HASHED)) store_key(T, (uint64_t)s, p, rev);
            lslot[e] = (int32_t)s | ((tag & HASHED) ? HASHED_SLOT : 0);
        }
    }
    __syncthreads();
    if (i < n) slots[i] = e >= 0 ? lslot[e] : -1;
}

// Round 0's verify over the whole batch.
__global__ __launch_bounds__(RB) void random_verify_kernel(ScgRandomTable T, ScgReads R, int64_t n, const int32_t* __restrict__ hits,
                                                           const int32_t* __restrict__ slots, int32_t* __restrict__ list_out,
                                                           int32_t* __restrict__ lens) {
    const int64_t i = (int64_t)blockIdx.x * RB + threadIdx.x;
    if (i >= n) return;
    const int32_t v = slots[i];
    if (v < 0 || !(v & HASHED_SLOT)) return;
    const uint64_t s = (uint64_t)(v & (HASHED_SLOT - 1));
    const uint8_t* p;
    bool rev;
    if (!locate(T, R, hits, i, p, rev)) return;
    if (!same_key(T, s, p, rev)) {
        atomicAdd(&T.counts[s], ~0ull);                      // -1
        list_out[atomicAdd(&lens[1], 1)] = (int32_t)i;
    }
}

// Round r >= 1, insert: the reads of list_in (lens[r] of them), one at a time (collisions are rare: no aggregation).
__global__ __launch_bounds__(RB) void random_round_insert_kernel(ScgRandomTable T, ScgReads R, const int32_t* __restrict__ hits,
                                                                 int32_t* __restrict__ slots, const int32_t* __restrict__ list_in,
                                                                 const int32_t* __restrict__ lens, int round) {
    const int32_t len = lens[round];
    for (int32_t k = blockIdx.x * RB + threadIdx.x; k < len; k += ROUND_GRID * RB) {
        const int32_t i = list_in[k];
        const uint8_t* p;
        bool rev;
        if (!locate(T, R, hits, i, p, rev)) { slots[i] = -1; continue; }
        int bad = 0;
        const unsigned long long tag = key_tag(T, p, rev, round, &bad);
        bool claimed = false;
        const int64_t s = tag ? table_insert(T, tag, 1ull, claimed) : -1;
        if (s < 0) { atomicAdd(&T.state[2], 1ull); slots[i] = -1; continue; }
        if (claimed) store_key(T, (uint64_t)s, p, rev);
        slots[i] = (int32_t)s | HASHED_SLOT;
    }
}

// Round r >= 1, verify: mismatching reads give back their count and go on to round r + 1, or after the last round
// count as unresolved (read-out reports them).
__global__ __launch_bounds__(RB) void random_round_verify_kernel(ScgRandomTable T, ScgReads R, const int32_t* __restrict__ hits,
                                                                 const int32_t* __restrict__ slots, const int32_t* __restrict__ list_in,
                                                                 int32_t* __restrict__ list_out, int32_t* __restrict__ lens, int round) {
    const int32_t len = lens[round];
    for (int32_t k = blockIdx.x * RB + threadIdx.x; k < len; k += ROUND_GRID * RB) {
        const int32_t i = list_in[k];
        const int32_t v = slots[i];
        if (v < 0) continue;
        const uint64_t s = (uint64_t)(v & (HASHED_SLOT - 1));
        const uint8_t* p;
        bool rev;
        if (!locate(T, R, hits, i, p, rev)) continue;
        if (same_key(T, s, p, rev)) continue;
        atomicAdd(&T.counts[s], ~0ull);
        if (round + 1 < SCG_RANDOM_ROUNDS) list_out[atomicAdd(&lens[round + 1], 1)] = i;
        else atomicAdd(&T.state[2], 1ull);
    }
}

__global__ __launch_bounds__(RB) void random_rehash_kernel(ScgRandomTable F, ScgRandomTable T) {
    const uint64_t cap = F.mask + 1;
    for (uint64_t s = (uint64_t)blockIdx.x * RB + threadIdx.x; s < cap; s += (uint64_t)gridDim.x * RB) {
        const unsigned long long tag = F.tags[s];
        if (!tag) continue;
        uint64_t t = fmix64(tag) & T.mask;
        for (uint64_t probe = 0; probe <= T.mask; ++probe) {
            if (atomicCAS(&T.tags[t], 0ull, tag) == 0) break;
            t = (t + 1) & T.mask;
        }
        T.counts[t] = F.counts[s];
        if (F.ids) T.ids[t] = F.ids[s];
        if (tag & HASHED) {
            const uint8_t* a = F.arena + s * (uint64_t)F.vlen;
            uint8_t* b = T.arena + t * (uint64_t)T.vlen;
            for (int j = 0; j < F.vlen; ++j) b[j] = a[j];
        }
    }
}

__global__ __launch_bounds__(RB) void random_compact_kernel(ScgRandomTable T, unsigned long long* __restrict__ packed_tags,
                                                            unsigned long long* __restrict__ packed_counts, int32_t* __restrict__ hashed_slots,
                                                            unsigned long long* __restrict__ hashed_counts, unsigned long long* __restrict__ n_out,
                                                            bool with_ids) {
    const uint64_t cap = T.mask + 1;
    for (uint64_t s = (uint64_t)blockIdx.x * RB + threadIdx.x; s < cap; s += (uint64_t)gridDim.x * RB) {
        const unsigned long long tag = T.tags[s];
        if (!tag) continue;
        const unsigned long long c = with_ids ? (unsigned long long)T.ids[s] : T.counts[s];
        if (!with_ids && !c) continue;
        if (tag & HASHED) {
            const unsigned long long k = atomicAdd(&n_out[1], 1ull);
            hashed_slots[k] = (int32_t)s; hashed_counts[k] = c;
        } else {
            const unsigned long long k = atomicAdd(&n_out[0], 1ull);
            packed_tags[k] = tag; packed_counts[k] = c;
        }
    }
}

// One pass over the slots, a wavefront on 64 neighbouring ones at a time (the trip count is the same for a whole
// workgroup, so every ballot sees all 64 lanes).  The lanes whose slot has a count take consecutive places in the list
// from one atomic add of their first lane.
__global__ __launch_bounds__(RB) void random_harvest_kernel(ScgRandomTable T, int32_t* __restrict__ list, uint32_t list_cap,
                                                            unsigned int* __restrict__ n_out) {
    const uint64_t cap = T.mask + 1;
    const int lane = (int)(threadIdx.x & (WAVE - 1));
    for (uint64_t base = (uint64_t)blockIdx.x * RB; base < cap; base += (uint64_t)gridDim.x * RB) {
        const uint64_t s = base + threadIdx.x;
        const unsigned long long c = s < cap ? T.counts[s] : 0ull;
        const unsigned long long takers = __ballot(c != 0);
        if (!takers) continue;
        const int first_lane = __ffsll(takers) - 1;
        unsigned int first = 0;
        if (lane == first_lane) first = atomicAdd(&n_out[0], (unsigned int)__popcll(takers));
        first = (unsigned int)__shfl((int)first, first_lane);
        if (c != 0) {
            const unsigned int k = first + (unsigned int)__popcll(takers & ((1ull << lane) - 1ull));
            if (c > 0x7FFFFFFFull || k >= list_cap) {
                atomicOr(&n_out[1], c > 0x7FFFFFFFull ? 1u : 2u);
            } else {
                list[2 * (size_t)k] = (int32_t)T.ids[s];
                list[2 * (size_t)k + 1] = (int32_t)c;
            }
            T.counts[s] = 0;
        }
    }
}

__global__ __launch_bounds__(RB) void random_decode_kernel(const unsigned long long* __restrict__ tags, int64_t n, int32_t vlen, char* __restrict__ out) {
    const int64_t k = (int64_t)blockIdx.x * RB + threadIdx.x;
    if (k >= n) return;
    const unsigned long long t = tags[k];
    char* o = out + k * (int64_t)(vlen + 1);
    for (int j = 0; j < vlen; ++j) o[j] = "ACGT"[(t >> (2 * (vlen - 1 - j))) & 3];
    o[vlen] = 0;
}

__global__ __launch_bounds__(RB) void random_gather_kernel(ScgRandomTable T, const int32_t* __restrict__ slots, int64_t n, uint8_t* __restrict__ out) {
    const int64_t k = (int64_t)blockIdx.x * RB + threadIdx.x;
    if (k >= n) return;
    const uint8_t* a = T.arena + (uint64_t)slots[k] * (uint64_t)T.vlen;
    uint8_t* o = out + k * (int64_t)T.vlen;
    for (int j = 0; j < T.vlen; ++j) o[j] = a[j];
}

inline unsigned blocks_for(int64_t n) { return (unsigned)((n + RB - 1) / RB); }
inline unsigned table_grid(uint64_t cap) { const uint64_t b = (cap + RB - 1) / RB; return (unsigned)(b < 8192 ? b : 8192); }

} // namespace

hipError_t launch_random_insert(const ScgRandomTable& T, const ScgReads& R, int64_t n, const int32_t* hits, int32_t* slots,
                                int64_t ordinal0, hipStream_t stream) {
    if (n <= 0) return hipSuccess;
    hipLaunchKernelGGL(random_insert_kernel, dim3(blocks_for(n)), dim3(RB), 0, stream, T, R, n, hits, slots, ordinal0);
    return hipGetLastError();
}

hipError_t launch_random_verify_rounds(const ScgRandomTable& T, const ScgReads& R, int64_t n, const int32_t* hits, int32_t* slots,
                                       int32_t* list_a, int32_t* list_b, int32_t* lens, hipStream_t stream) {
    if (n <= 0) return hipSuccess;
    hipLaunchKernelGGL(random_verify_kernel, dim3(blocks_for(n)), dim3(RB), 0, stream, T, R, n, hits, slots, list_a, lens);
    for (int r = 1; r < SCG_RANDOM_ROUNDS; ++r) {
        int32_t* in = (r & 1) ? list_a : list_b;
        int32_t* out = (r & 1) ? list_b : list_a;
        hipLaunchKernelGGL(random_round_insert_kernel, dim3(ROUND_GRID), dim3(RB), 0, stream, T, R, hits, slots, in, lens, r);
        hipLaunchKernelGGL(random_round_verify_kernel, dim3(ROUND_GRID), dim3(RB), 0, stream, T, R, hits, slots, in, out, lens, r);
    }
    return hipGetLastError();
}

hipError_t launch_random_rehash(const ScgRandomTable& from, const ScgRandomTable& to, hipStream_t stream) {
    hipLaunchKernelGGL(random_rehash_kernel, dim3(table_grid(from.mask + 1)), dim3(RB), 0, stream, from, to);
    return hipGetLastError();
}

hipError_t launch_random_compact(const ScgRandomTable& T, unsigned long long* packed_tags, unsigned long long* packed_counts,
                                 int32_t* hashed_slots, unsigned long long* hashed_counts, unsigned long long* n_out, bool with_ids,
                                 hipStream_t stream) {
    if (with_ids && !T.ids) return hipErrorInvalidValue;
    hipLaunchKernelGGL(random_compact_kernel, dim3(table_grid(T.mask + 1)), dim3(RB), 0, stream, T, packed_tags, packed_counts,
                       hashed_slots, hashed_counts, n_out, with_ids);
    return hipGetLastError();
}

hipError_t launch_random_harvest(const ScgRandomTable& T, int32_t* list, uint32_t list_cap, unsigned int* n_out, hipStream_t stream) {
    if (!T.ids) return hipErrorInvalidValue;
    hipLaunchKernelGGL(random_harvest_kernel, dim3(table_grid(T.mask + 1)), dim3(RB), 0, stream, T, list, list_cap, n_out);
    return hipGetLastError();
}

size_t random_sort_scratch_bytes(size_t n) {
    size_t bytes = 0;
    unsigned long long* k = nullptr;
    if (rocprim::radix_sort_pairs(nullptr, bytes, k, k, k, k, n, 0, 64, nullptr) != hipSuccess) return 0;
    return bytes + 256;
}

hipError_t launch_random_sort(const unsigned long long* keys_in, unsigned long long* keys_out, const unsigned long long* vals_in,
                              unsigned long long* vals_out, size_t n, int end_bit, void* scratch, size_t scratch_bytes, hipStream_t stream) {
    if (n == 0) return hipSuccess;
    size_t bytes = scratch_bytes;
    return rocprim::radix_sort_pairs(scratch, bytes, keys_in, keys_out, vals_in, vals_out, n, 0, end_bit, stream);
}

hipError_t launch_random_decode(const unsigned long long* tags, int64_t n, int32_t vlen, char* out, hipStream_t stream) {
    if (n <= 0) return hipSuccess;
    hipLaunchKernelGGL(random_decode_kernel, dim3(blocks_for(n)), dim3(RB), 0, stream, tags, n, vlen, out);
    return hipGetLastError();
}

hipError_t launch_random_gather(const ScgRandomTable& T, const int32_t* slots, int64_t n, uint8_t* out, hipStream_t stream) {
    if (n <= 0) return hipSuccess;
    hipLaunchKernelGGL(random_gather_kernel, dim3(blocks_for(n)), dim3(RB), 0, stream, T, slots, n, out);
    return hipGetLastError();
}

} // namespace scg
