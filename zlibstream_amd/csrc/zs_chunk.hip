// zs_chunk.hip -- KN, the kernels of the chunked-array calls (zs_chunk.h holds the geometry and the per-lane step):
//   zs_chunk_place_kernel    inflated chunks -> the array: unshuffle and placement in one pass; missing chunks write `fill`
//   zs_chunk_gather_kernel   the inverse: the clipped region read, padded with `fill`, written shuffled or plain
//   zs_chunk_survey_kernel   per item, whether its existing elements all equal `fill`; zs_chunk_fold_kernel folds a chunk's records
// The first three run over the flat list of the call's items, one wave an item: a stretch of one row of one chunk, in passes
// of 64 lanes x `unit` elements.  A lane reads `unit` bytes of each of the elem_size planes (one 16-byte load a plane where
// unit is 16: lane i at base + 16 i), interleaves them in registers and writes its unit * elem_size contiguous bytes with
// 16-byte stores.  No atomics, no LDS, and every output byte has one writer.
#pragma once

#include <hip/hip_runtime.h>

#include "zs_chunk.h"
#include "zs_png.h"

namespace zs {

constexpr int kChunkItemsPerWg = 4;

// the flat item `first + (this wave's place in the grid)` of the launch: its job and its item there, false behind the list
__device__ __forceinline__ bool chunk_my_item(const int32_t *item_off, int n, int64_t first, int *job, int64_t *q) {
    const int64_t item = first + (int64_t)blockIdx.x * kChunkItemsPerWg + (threadIdx.x >> 6);
    if (item >= item_off[n]) return false;
    *job = __builtin_amdgcn_readfirstlane(png_row_image(item_off, n, item));
    *q = item - item_off[*job];
    return true;
}

__global__ __launch_bounds__(64 * kChunkItemsPerWg) void zs_chunk_place_kernel(const ChunkJob *__restrict__ jobs, const int32_t *__restrict__ item_off, int n, int64_t first,
                                                                                 const ChunkGeom *__restrict__ geoms) {
    int j;
    int64_t q;
    if (!chunk_my_item(item_off, n, first, &j, &q)) return;
    const ChunkJob &jb = jobs[j];  // (read where it lies: j is the wave's, so these are scalar loads, and no copy is indexed in private memory)
    chunk_place_item(geoms[jb.geom], jb, q, (int)threadIdx.x & 63);
}

__global__ __launch_bounds__(64 * kChunkItemsPerWg) void zs_chunk_gather_kernel(const ChunkJob *__restrict__ jobs, const int32_t *__restrict__ item_off, int n, int64_t first,
                                                                                  const ChunkGeom *__restrict__ geoms) {
    int j;
    int64_t q;
    if (!chunk_my_item(item_off, n, first, &j, &q)) return;
    const ChunkJob &jb = jobs[j];  // (read where it lies: j is the wave's, so these are scalar loads, and no copy is indexed in private memory)
    chunk_gather_item(geoms[jb.geom], jb, q, (int)threadIdx.x & 63);
}

// rec[item]: 1 where every existing element of the item is `fill`
__global__ __launch_bounds__(64 * kChunkItemsPerWg) void zs_chunk_survey_kernel(const ChunkJob *__restrict__ jobs, const int32_t *__restrict__ item_off, int n, int64_t first,
                                                                                  const ChunkGeom *__restrict__ geoms, uint8_t *__restrict__ rec) {
    int j;
    int64_t q;
    if (!chunk_my_item(item_off, n, first, &j, &q)) return;
    const ChunkJob &jb = jobs[j];  // (read where it lies: j is the wave's, so these are scalar loads, and no copy is indexed in private memory)
    const bool same = chunk_survey_item(geoms[jb.geom], jb, q, (int)threadIdx.x & 63);
    const bool all = __all(same);
    if ((threadIdx.x & 63) == 0) rec[item_off[j] + q] = all ? 1 : 0;
}

// flag[j]: 1 where all records of job j are; a wave a job
__global__ __launch_bounds__(64 * kChunkItemsPerWg) void zs_chunk_fold_kernel(const int32_t *__restrict__ item_off, int n, const uint8_t *__restrict__ rec, uint8_t *__restrict__ flag) {
    const int j = (int)blockIdx.x * kChunkItemsPerWg + (int)(threadIdx.x >> 6);
    if (j >= n) return;
    bool same = true;
    for (int64_t k = (int64_t)item_off[j] + (threadIdx.x & 63); k < item_off[j + 1]; k += 64) same = same && rec[k] != 0;
    const bool all = __all(same);
    if ((threadIdx.x & 63) == 0) flag[j] = all ? 1 : 0;
}

}  // namespace zs
