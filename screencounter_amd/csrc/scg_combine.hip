// scg_combine.hip -- combination counts of many files as one matrix: combineComboCounts (R/combineComboCounts.R:31-57)
// on the device.
//
// Two steps, both on 64-bit keys (first << 32 | second):
//   1. a file's dense histogram -> its non-zero cells as sorted (key, count) pairs, so that K_f pairs cross the link and
//      not n0 * n1 cells.  Cell order is key order, so a stream compaction is all it takes: count the non-zero cells of
//      every tile, scan the tile counts (rocPRIM), and scatter every non-zero cell to tile offset + its rank in the tile.
//      The rank comes from wave ballots and a scan of the wave counts through LDS: no atomics, and no workgroup waits
//      for another -- the order, and with it the determinism, is the scan's.
//   2. the union of the files' keys (launch_sort_rle of scg_sparse.hip gives the distinct keys, ascending) and, per
//      entry, its row: a lower bound over the distinct keys.
// A tile is SCG_COMPACT_TILE_CELLS cells: 256 lanes x 4 loads of 16 bytes, load j of lane t taking cells
// 4 * (256 j + t) .. + 3 of the tile, so that every load of a wave is one contiguous KiB.  Tile order is therefore
// (load, wave, lane, component): sixteen (load, wave) segments, whose counts are scanned through LDS.
#include <cstring>

#include <hip/hip_runtime.h>
#include <rocprim/rocprim.hpp>

#include "scg_launch.h"

namespace scg {

namespace {

constexpr int COMPACT_BLOCK = 256;
constexpr int COMPACT_WAVES = COMPACT_BLOCK / 64;
constexpr int COMPACT_LOADS = SCG_COMPACT_TILE_CELLS / (4 * COMPACT_BLOCK);
static_assert(COMPACT_LOADS * 4 * COMPACT_BLOCK == SCG_COMPACT_TILE_CELLS, "a tile is a whole number of 16-byte loads per lane");

// Cells 4 v .. 4 v + 3 (v: 16-byte vector number within the whole array); cells at or past n_cells read as zero.
__device__ __forceinline__ int4 load_cells(const int32_t* __restrict__ cells, uint64_t v, uint64_t n_cells) {
    const uint64_t c = v * 4;
    if (c + 4 <= n_cells) return *reinterpret_cast<const int4*>(cells + c);
    int4 x = make_int4(0, 0, 0, 0);
    if (c < n_cells) x.x = cells[c];
    if (c + 1 < n_cells) x.y = cells[c + 1];
    if (c + 2 < n_cells) x.z = cells[c + 2];
    return x;
}

// Non-zero cells of the (load, wave) segment this wave holds in x: wave-uniform.
__device__ __forceinline__ uint32_t segment_count(const int4& x) {
    return static_cast<uint32_t>(__popcll(__ballot(x.x != 0)) + __popcll(__ballot(x.y != 0)) + __popcll(__ballot(x.z != 0)) +
                                 __popcll(__ballot(x.w != 0)));
}

__global__ void __launch_bounds__(COMPACT_BLOCK) combo_compact_count_kernel(const int32_t* __restrict__ cells, uint64_t n_cells,
                                                                           unsigned long long* __restrict__ tile_counts) {
    __shared__ uint32_t wave_count[COMPACT_WAVES];
    const uint64_t tile = blockIdx.x;
    const uint64_t v0 = tile * (SCG_COMPACT_TILE_CELLS / 4) + threadIdx.x;
    int4 x[COMPACT_LOADS];
#pragma unroll
    for (int j = 0; j < COMPACT_LOADS; ++j) x[j] = load_cells(cells, v0 + static_cast<uint64_t>(j) * COMPACT_BLOCK, n_cells);
    uint32_t n = 0;
#pragma unroll
    for (int j = 0; j < COMPACT_LOADS; ++j) n += segment_count(x[j]);
    if ((threadIdx.x & 63) == 0) wave_count[threadIdx.x >> 6] = n;
    __syncthreads();
    if (threadIdx.x == 0) {
        uint32_t t = 0;
#pragma unroll
        for (int w = 0; w < COMPACT_WAVES; ++w) t += wave_count[w];
        tile_counts[tile] = t;
    }
}

__global__ void __launch_bounds__(COMPACT_BLOCK) combo_compact_scatter_kernel(const int32_t* __restrict__ cells, uint64_t n_cells, uint32_t n1,
                                                                             const unsigned long long* __restrict__ tile_offsets,
                                                                             uint64_t* __restrict__ keys_out, int32_t* __restrict__ counts_out) {
    __shared__ uint32_t seg_count[COMPACT_LOADS * COMPACT_WAVES];
    const uint64_t tile = blockIdx.x;
    const uint64_t v0 = tile * (SCG_COMPACT_TILE_CELLS / 4) + threadIdx.x;
    const int wave = threadIdx.x >> 6;
    int4 x[COMPACT_LOADS];
#pragma unroll
    for (int j = 0; j < COMPACT_LOADS; ++j) x[j] = load_cells(cells, v0 + static_cast<uint64_t>(j) * COMPACT_BLOCK, n_cells);
    // rank of this lane's first non-zero cell of load j within its (load, wave) segment: the cells of the lanes below
    uint32_t below[COMPACT_LOADS];
#pragma unroll
    for (int j = 0; j < COMPACT_LOADS; ++j) {
        const unsigned long long b0 = __ballot(x[j].x != 0), b1 = __ballot(x[j].y != 0), b2 = __ballot(x[j].z != 0), b3 = __ballot(x[j].w != 0);
        const unsigned long long lower = (1ull << (threadIdx.x & 63)) - 1;
        below[j] = static_cast<uint32_t>(__popcll(b0 & lower) + __popcll(b1 & lower) + __popcll(b2 & lower) + __popcll(b3 & lower));
        const uint32_t n = static_cast<uint32_t>(__popcll(b0) + __popcll(b1) + __popcll(b2) + __popcll(b3));
        if ((threadIdx.x & 63) == 0) seg_count[j * COMPACT_WAVES + wave] = n;
    }
    __syncthreads();                                        // (every lane of every tile arrives: nothing above returns)
    const unsigned long long base = tile_offsets[tile];
    uint32_t seg[COMPACT_LOADS * COMPACT_WAVES];
#pragma unroll
    for (int s = 0; s < COMPACT_LOADS * COMPACT_WAVES; ++s) seg[s] = seg_count[s];
#pragma unroll
    for (int j = 0; j < COMPACT_LOADS; ++j) {
        uint32_t before = 0;                                // the segments before (load j, this wave)
#pragma unroll
        for (int s = 0; s < COMPACT_LOADS * COMPACT_WAVES; ++s) before += s < j * COMPACT_WAVES + wave ? seg[s] : 0;
        if ((x[j].x | x[j].y | x[j].z | x[j].w) == 0) continue;
        const uint64_t c0 = (v0 + static_cast<uint64_t>(j) * COMPACT_BLOCK) * 4;     // 64-bit cell number, 32-bit halves of the key
        uint32_t first = static_cast<uint32_t>(c0 / n1), second = static_cast<uint32_t>(c0 % n1);
        unsigned long long at = base + before + below[j];
        const int32_t v[4] = {x[j].x, x[j].y, x[j].z, x[j].w};
#pragma unroll
        for (int c = 0; c < 4; ++c) {
            if (v[c] != 0) {
                keys_out[at] = (static_cast<uint64_t>(first) << 32) | second;
                counts_out[at] = v[c];
                ++at;
            }
            if (++second == n1) { second = 0; ++first; }
        }
    }
}

// Lower bound of every key among the distinct keys; their number is read on the device (the run-length encode that made
// them is still in flight when this is enqueued).
__global__ void __launch_bounds__(256) combo_union_rows_kernel(const uint64_t* __restrict__ keys, uint64_t n, const uint64_t* __restrict__ unique,
                                                               const uint32_t* __restrict__ n_unique, int32_t* __restrict__ rows_out,
                                                               int32_t* __restrict__ flag) {
    const uint64_t i = static_cast<uint64_t>(blockIdx.x) * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const uint64_t key = keys[i];
    uint64_t base = 0, len = *n_unique;
    if (len == 0) { *flag = 1; return; }
    while (len > 1) {
        const uint64_t half = len >> 1;
        base += unique[base + half - 1] < key ? half : 0;
        len -= half;
    }
    base += unique[base] < key ? 1 : 0;
    if (base >= *n_unique || unique[base] != key) { *flag = 1; return; }
    rows_out[i] = static_cast<int32_t>(base);
}

__global__ void __launch_bounds__(256) combo_equal_neighbours_kernel(const uint64_t* __restrict__ keys, uint64_t n, int32_t* __restrict__ flag) {
    const uint64_t i = static_cast<uint64_t>(blockIdx.x) * blockDim.x + threadIdx.x + 1;
    if (i < n && keys[i] == keys[i - 1]) *flag = 1;
}

inline unsigned int blocks_for(uint64_t n, unsigned int block) { return static_cast<unsigned int>((n + block - 1) / block); }

} // namespace

size_t compact_scan_scratch_bytes(uint64_t n_cells) {
    size_t bytes = 0;
    unsigned long long* p = nullptr;
    if (rocprim::exclusive_scan(nullptr, bytes, p, p, 0ull, static_cast<size_t>(compact_tiles(n_cells) + 1), rocprim::plus<unsigned long long>(), nullptr) !=
        hipSuccess) {
        return 0;
    }
    return bytes + 256;
}

hipError_t launch_compact_count(const int32_t* cells, uint64_t n_cells, unsigned long long* d_tile_counts, unsigned long long* d_tile_offsets,
                                void* d_scratch, size_t scratch_bytes, hipStream_t stream) {
    const uint64_t tiles = compact_tiles(n_cells);
    if ((reinterpret_cast<uintptr_t>(cells) & 15) != 0 || tiles > 0x7FFFFFFFull) return hipErrorInvalidValue;
    hipError_t e = hipMemsetAsync(d_tile_counts + tiles, 0, sizeof(unsigned long long), stream);
    if (e != hipSuccess) return e;
    if (tiles) {
        hipLaunchKernelGGL(combo_compact_count_kernel, dim3(static_cast<unsigned int>(tiles)), dim3(COMPACT_BLOCK), 0, stream, cells, n_cells, d_tile_counts);
        e = hipGetLastError();
        if (e != hipSuccess) return e;
    }
    size_t bytes = scratch_bytes;
    return rocprim::exclusive_scan(d_scratch, bytes, d_tile_counts, d_tile_offsets, 0ull, static_cast<size_t>(tiles + 1),
                                   rocprim::plus<unsigned long long>(), stream);
}

hipError_t launch_compact_scatter(const int32_t* cells, uint64_t n_cells, uint32_t n1, const unsigned long long* d_tile_offsets,
                                  uint64_t* keys_out, int32_t* counts_out, hipStream_t stream) {
    const uint64_t tiles = compact_tiles(n_cells);
    if ((reinterpret_cast<uintptr_t>(cells) & 15) != 0 || tiles > 0x7FFFFFFFull || n1 == 0) return hipErrorInvalidValue;
    if (tiles == 0) return hipSuccess;
    hipLaunchKernelGGL(combo_compact_scatter_kernel, dim3(static_cast<unsigned int>(tiles)), dim3(COMPACT_BLOCK), 0, stream, cells, n_cells, n1,
                       d_tile_offsets, keys_out, counts_out);
    return hipGetLastError();
}

hipError_t launch_union_rows(const uint64_t* keys, uint64_t n, const uint64_t* d_unique, const uint32_t* d_n_unique, int32_t* rows_out,
                             int32_t* d_flag, hipStream_t stream) {
    if (n == 0) return hipSuccess;
    if (n > 0xFFFFFFFFull) return hipErrorInvalidValue;
    hipLaunchKernelGGL(combo_union_rows_kernel, dim3(blocks_for(n, 256)), dim3(256), 0, stream, keys, n, d_unique, d_n_unique, rows_out, d_flag);
    return hipGetLastError();
}

size_t sort_pairs_scratch_bytes(size_t n) {
    size_t bytes = 0;
    uint64_t* k = nullptr;
    int32_t* v = nullptr;
    if (rocprim::radix_sort_pairs(nullptr, bytes, k, k, v, v, n, 0, 64, nullptr) != hipSuccess) return 0;
    return bytes + 256;
}

hipError_t launch_sort_pairs(const uint64_t* keys_in, uint64_t* keys_out, const int32_t* vals_in, int32_t* vals_out, size_t n,
                             void* d_scratch, size_t scratch_bytes, hipStream_t stream) {
    if (n == 0) return hipSuccess;
    size_t bytes = scratch_bytes;
    return rocprim::radix_sort_pairs(d_scratch, bytes, keys_in, keys_out, vals_in, vals_out, n, 0, 64, stream);
}

hipError_t launch_flag_equal_neighbours(const uint64_t* keys, uint64_t n, int32_t* d_flag, hipStream_t stream) {
    if (n < 2) return hipSuccess;
    if (n > 0xFFFFFFFFull) return hipErrorInvalidValue;
    hipLaunchKernelGGL(combo_equal_neighbours_kernel, dim3(blocks_for(n - 1, 256)), dim3(256), 0, stream, keys, n, d_flag);
    return hipGetLastError();
}

} // namespace scg
