// zs_chunk.hip -- KN, the kernels of the chunked-array calls (zs_chunk.h holds the geometry and the per-lane step):
//   zs_chunk_place_kernel    inflated chunks -> the array: unshuffle and placement in one pass; missing chunks write `fill`
//   zs_chunk_gather_kernel   the inverse: the clipped region read, padded with `fill`, written shuffled or plain
//   zs_chunk_survey_kernel   per item, whether its existing elements all equal `fill`; zs_chunk_fold_kernel folds a chunk's records
// The first three run over the flat list of the call's items, one wave an item: a stretch of one row of one chunk, in passes
// of 64 lanes x `unit` elements.  A lane reads `unit` bytes of each of the elem_size planes (one 16-byte load a plane where
// unit is 16: lane i at base + 16 i), interleaves them in registers and writes its unit * elem_size contiguous bytes with
// 16-byte stores.  No atomics, no LDS, and every output byte has one writer.  A job whose elements lie big-endian in the chunk
// (kJobSwap) takes plane elem_size - 1 - j where it took plane j, and reverses the bytes of a plain chunk's elements in registers.
// Behind them KL (Fletcher-32 of many spans: a tile launch and a fold) and KI (the delta filter: an encode launch; for decode
// tile sums, their scan and a second pass), over the same flat lists.
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

// ------------------------------------------------------------------ Fletcher-32 (KL) and delta (KI), zs_chunk.h's steps
// The same flat lists, a wave an item.  KL: an item is a tile of kFletTile bytes of a span; the lanes read the tile in 16-byte
// words aligned in memory (the bytes of the first and last word outside the tile do not count), keep 64-bit sums, reduce them
// modulo 65535 and add them across the wave with shuffles; lane 0 stores the tile's record with one 16-byte store.  The fold, a
// wave a span, adds the records by the combine rule -- a2 + (words behind the tile) a1 -- and writes the checksum.
__device__ __forceinline__ uint32_t chunk_wave_sum(uint32_t v) {
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) v += __shfl_xor(v, d, 64);
    return v;
}
__device__ __forceinline__ uint64_t chunk_wave_sum64(uint64_t v) {
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) v += (uint64_t)__shfl_xor((unsigned long long)v, d, 64);
    return v;
}

__global__ __launch_bounds__(64 * kChunkItemsPerWg) void zs_fletcher_tile_kernel(const FletSpan *__restrict__ spans, const int32_t *__restrict__ tile_off, int n, int64_t first,
                                                                                   FletSum *__restrict__ rec) {
    int si;
    int64_t q;
    if (!chunk_my_item(tile_off, n, first, &si, &q)) return;
    const FletSpan &sp = spans[si];
    const int64_t t0 = q * kFletTile;
    const int len = (int)(sp.len - t0 < kFletTile ? sp.len - t0 : kFletTile);
    const uintptr_t a0 = (uintptr_t)sp.src + (uintptr_t)t0;
    const int h = (int)(a0 & 15), lane = (int)threadIdx.x & 63;
    uint64_t A1 = 0, A2 = 0;
    fletcher_tile_lane((const uint8_t *)(a0 - (uintptr_t)h), h, len, lane, &A1, &A2);
    const bool nz = __any(A1 != 0);
    const uint32_t a1 = chunk_wave_sum((uint32_t)(A1 % 65535u)) % 65535u, a2 = chunk_wave_sum((uint32_t)(A2 % 65535u)) % 65535u;
    if (lane == 0) {
        uint4 r = make_uint4(a1, a2, nz ? 1u : 0u, 0u);
        *(uint4 *)(rec + tile_off[si] + q) = r;
    }
}

__global__ __launch_bounds__(64 * kChunkItemsPerWg) void zs_fletcher_fold_kernel(const FletSpan *__restrict__ spans, const int32_t *__restrict__ tile_off, int n,
                                                                                   const FletSum *__restrict__ rec, uint32_t *__restrict__ out) {
    const int si = (int)blockIdx.x * kChunkItemsPerWg + (int)(threadIdx.x >> 6);
    if (si >= n) return;
    const int lane = (int)threadIdx.x & 63;
    const int64_t len = spans[si].len, words = (len + 1) / 2;
    const int tiles = tile_off[si + 1] - tile_off[si];
    uint64_t B1 = 0, B2 = 0;
    uint32_t any = 0;
    for (int t = lane; t < tiles; t += 64) {
        const FletSum r = rec[tile_off[si] + t];
        const int64_t behind = t + 1 < tiles ? words - (int64_t)(t + 1) * (kFletTile / 2) : 0;
        B1 += r.a1, B2 += r.a2 + (uint64_t)(behind % 65535) * r.a1, any |= r.nz;
    }
    FletSum s;
    s.a1 = chunk_wave_sum((uint32_t)(B1 % 65535u)) % 65535u, s.a2 = chunk_wave_sum((uint32_t)(B2 % 65535u)) % 65535u;
    s.nz = __any(any != 0) ? 1u : 0u, s.pad = 0;
    if (lane == 0) {
        const uint32_t v = fletcher_finish(s);
        out[si] = v;
        uint8_t *d = spans[si].dst;
        if (d) d[0] = (uint8_t)v, d[1] = (uint8_t)(v >> 8), d[2] = (uint8_t)(v >> 16), d[3] = (uint8_t)(v >> 24);
    }
}

// KI.  An item is a tile of kDeltaTile elements of a job, in kDeltaPasses passes of 64 lanes x 16 elements.  Encode reads plain
// elements and writes the differences big-endian and in planes where the job says so.  Decode is a prefix sum in three
// launches: the tiles' sums (the load side unshuffles and reverses), an exclusive scan of a job's tile sums by one wave, and the
// tiles again, each from its carry: a lane's 16 running sums, the lanes' totals scanned across the wave with shuffles.
#define ZS_DELTA_ES(es, CALL) \
    if (es == 1) { constexpr int ES = 1; CALL; } else if (es == 2) { constexpr int ES = 2; CALL; } else if (es == 4) { constexpr int ES = 4; CALL; } else { constexpr int ES = 8; CALL; }

__global__ __launch_bounds__(64 * kChunkItemsPerWg) void zs_delta_encode_kernel(const DeltaJob *__restrict__ jobs, const int32_t *__restrict__ tile_off, int n, int64_t first) {
    int j;
    int64_t t;
    if (!chunk_my_item(tile_off, n, first, &j, &t)) return;
    const DeltaJob &jb = jobs[j];
    const int lane = (int)threadIdx.x & 63;
    for (int pass = 0; pass < kDeltaPasses; pass++) {
        ZS_DELTA_ES(jb.es, delta_encode_lane<ES>(jb, t, pass, lane));
    }
    delta_copy_left(jb, t, lane);
}

__global__ __launch_bounds__(64 * kChunkItemsPerWg) void zs_delta_sum_kernel(const DeltaJob *__restrict__ jobs, const int32_t *__restrict__ tile_off, int n, int64_t first,
                                                                               uint64_t *__restrict__ sums) {
    int j;
    int64_t t;
    if (!chunk_my_item(tile_off, n, first, &j, &t)) return;
    const DeltaJob &jb = jobs[j];
    const int lane = (int)threadIdx.x & 63;
    uint64_t sum = 0;
    for (int pass = 0; pass < kDeltaPasses; pass++) {
        uint64_t x[kDeltaUnit];
        int64_t e;
        int cnt;
        ZS_DELTA_ES(jb.es, sum += delta_decode_load<ES>(jb, t, pass, lane, x, &e, &cnt));
    }
    sum = chunk_wave_sum64(sum);
    if (lane == 0) sums[tile_off[j] + t] = sum;
}

// sums[tile] becomes the sum of the job's tiles in front of it; a wave a job
__global__ __launch_bounds__(64 * kChunkItemsPerWg) void zs_delta_scan_kernel(const int32_t *__restrict__ tile_off, int n, uint64_t *__restrict__ sums) {
    const int j = (int)blockIdx.x * kChunkItemsPerWg + (int)(threadIdx.x >> 6);
    if (j >= n) return;
    const int lane = (int)threadIdx.x & 63, tiles = tile_off[j + 1] - tile_off[j];
    uint64_t *s = sums + tile_off[j], carry = 0;
    for (int base = 0; base < tiles; base += 64) {
        const uint64_t v = base + lane < tiles ? s[base + lane] : 0;
        uint64_t incl = v;
#pragma unroll
        for (int d = 1; d < 64; d <<= 1) {
            const uint64_t up = (uint64_t)__shfl_up((unsigned long long)incl, d, 64);
            if (lane >= d) incl += up;
        }
        if (base + lane < tiles) s[base + lane] = carry + incl - v;
        carry += (uint64_t)__shfl((unsigned long long)incl, 63, 64);
    }
}

__global__ __launch_bounds__(64 * kChunkItemsPerWg) void zs_delta_decode_kernel(const DeltaJob *__restrict__ jobs, const int32_t *__restrict__ tile_off, int n, int64_t first,
                                                                                  const uint64_t *__restrict__ sums) {
    int j;
    int64_t t;
    if (!chunk_my_item(tile_off, n, first, &j, &t)) return;
    const DeltaJob &jb = jobs[j];
    const int lane = (int)threadIdx.x & 63;
    uint64_t carry = sums[tile_off[j] + t];
    for (int pass = 0; pass < kDeltaPasses; pass++) {
        uint64_t x[kDeltaUnit];
        int64_t e = 0;
        int cnt = 0;
        uint64_t mine = 0;
        ZS_DELTA_ES(jb.es, mine = delta_decode_load<ES>(jb, t, pass, lane, x, &e, &cnt));
        uint64_t incl = mine;
#pragma unroll
        for (int d = 1; d < 64; d <<= 1) {
            const uint64_t up = (uint64_t)__shfl_up((unsigned long long)incl, d, 64);
            if (lane >= d) incl += up;
        }
        ZS_DELTA_ES(jb.es, delta_decode_store<ES>(jb, e, cnt, x, carry + incl - mine));
        carry += (uint64_t)__shfl((unsigned long long)incl, 63, 64);
    }
    delta_copy_left(jb, t, lane);
}

}  // namespace zs
