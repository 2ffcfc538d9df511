// zs_exr.hip -- KE, the predictor kernels of the OpenEXR calls (zs_exr.h holds the container's rules and the per-lane step):
//   zs_exr_reduce_kernel   one byte sum per segment (kExrSeg bytes) of each half of every chunk's stored bytes
//   zs_exr_undo_kernel     stored bytes -> channel planes: the running sum over the whole chunk, the two halves interleaved,
//                          the raw bytes scattered to their (row, channel) runs
//   zs_exr_predict_kernel  the inverse: runs gathered, split into halves, differenced
// All three run over the flat list of the call's tiles, one wave a tile: kExrTile output bytes of one chunk, that is bytes
// [a, a + kExrSeg) of each half, in passes of 64 lanes x 16 bytes of each.  A tile's two carries are the sums of the segment
// bytes in front of it, which the reduce launch has written: no workgroup waits for another.  No atomics, no LDS, and every
// output byte has one writer.
#pragma once

#include <hip/hip_runtime.h>

#include "zs_exr.h"
#include "zs_png.h"
#include "zs_tiff.hip"

namespace zs {

constexpr int kExrTilesPerWg = 4;

// the flat tile `first + (this wave's place in the grid)` of the launch: its job and its tile there, false behind the list
__device__ __forceinline__ bool exr_my_tile(const int32_t *tile_off, int n, int64_t first, int *job, int *q) {
    const int64_t tile = first + (int64_t)blockIdx.x * kExrTilesPerWg + (threadIdx.x >> 6);
    if (tile >= tile_off[n]) return false;
    *job = __builtin_amdgcn_readfirstlane(png_row_image(tile_off, n, tile));
    *q = __builtin_amdgcn_readfirstlane((int)(tile - tile_off[*job]));
    return true;
}

// 16 bytes at p + pos, of which only those in front of `end` exist (the others read as zero / are not written)
__device__ __forceinline__ void exr_load16(const uint8_t *p, int64_t pos, int64_t end, uint32_t w[4]) {
    w[0] = w[1] = w[2] = w[3] = 0;
    if (pos + 16 <= end) {
        const tiff_u32x4 v = *(const tiff_u32x4_a1 *)(p + pos);
        w[0] = v.x, w[1] = v.y, w[2] = v.z, w[3] = v.w;
    } else {
        for (int64_t b = pos; b < end; b++) w[(b - pos) >> 2] |= (uint32_t)p[b] << (8 * ((b - pos) & 3));
    }
}
__device__ __forceinline__ void exr_store16(uint8_t *p, int64_t pos, int64_t end, const uint32_t w[4]) {
    if (pos + 16 <= end) {
        tiff_u32x4 v;
        v.x = w[0], v.y = w[1], v.z = w[2], v.w = w[3];
        *(tiff_u32x4_a1 *)(p + pos) = v;
    } else {
        for (int64_t b = pos; b < end; b++) p[b] = (uint8_t)(w[(b - pos) >> 2] >> (8 * ((b - pos) & 3)));
    }
}

// Segment sums.  The wave of tile q sums bytes [a, a + kExrSeg) of the first half into seg[2 * tile_off[job] + q] and those of
// the second half, counted from h, into seg[2 * tile_off[job] + n_tiles + q].
__global__ __launch_bounds__(64 * kExrTilesPerWg) void zs_exr_reduce_kernel(const ExrJob *__restrict__ jobs, const int32_t *__restrict__ tile_off, int n, int64_t first,
                                                                               uint8_t *__restrict__ seg) {
    int j, q;
    if (!exr_my_tile(tile_off, n, first, &j, &q)) return;
    const ExrJob jb = jobs[j];
    if (jb.plain) return;
    const int lane = (int)threadIdx.x & 63;
    const int64_t U = jb.len, h = (U + 1) >> 1, a = (int64_t)q * kExrSeg;
    const int n_tiles = tile_off[j + 1] - tile_off[j];
    uint32_t s1 = 0, s2 = 0;
    for (int64_t pos = a + 16 * lane; pos < a + kExrSeg; pos += kExrPass) {
        uint32_t w[4];
        if (pos < h) {
            exr_load16(jb.t, pos, h, w);
            s1 = exr_add8(s1, exr_group_sum(w));
        }
        if (pos < U - h) {
            exr_load16(jb.t + h, pos, U - h, w);
            s2 = exr_add8(s2, exr_group_sum(w));
        }
    }
    s1 = tiff_wave_sum(exr_fold8(s1) & 0xFF), s2 = tiff_wave_sum(exr_fold8(s2) & 0xFF);
    if (lane == 0) {
        uint8_t *out = seg + 2 * (int64_t)tile_off[j];
        out[q] = (uint8_t)s1, out[n_tiles + q] = (uint8_t)s2;
    }
}

// 16 raw bytes of the chunk from `pos` on (`cnt` of them exist, 1 .. 16) to where the runs say; *r is the run of `pos` and is
// moved on.  One store where they lie in one run, else byte by byte.
__device__ __forceinline__ void exr_scatter16(const ExrRun *__restrict__ runs, int *r, int64_t pos, int cnt, const uint32_t w[4]) {
    ExrRun run = runs[*r];
    if (cnt == 16 && pos + 16 <= (int64_t)run.off + run.len) {
        tiff_u32x4 v;
        v.x = w[0], v.y = w[1], v.z = w[2], v.w = w[3];
        *(tiff_u32x4_a1 *)(run.p + (pos - run.off)) = v;
        if (pos + 16 == (int64_t)run.off + run.len) ++*r;
        return;
    }
#pragma unroll
    for (int b = 0; b < 16; b++) {
        if (b < cnt) {
            if (pos + b >= (int64_t)run.off + run.len) run = runs[++*r];
            run.p[pos + b - run.off] = (uint8_t)(w[b >> 2] >> (8 * (b & 3)));
        }
    }
    if (pos + cnt == (int64_t)run.off + run.len) ++*r;  // (the last run's end is the chunk's: nobody goes on from there)
}
// ... and the gather
__device__ __forceinline__ void exr_gather16(const ExrRun *__restrict__ runs, int *r, int64_t pos, int cnt, uint32_t w[4]) {
    ExrRun run = runs[*r];
    w[0] = w[1] = w[2] = w[3] = 0;
    if (cnt == 16 && pos + 16 <= (int64_t)run.off + run.len) {
        const tiff_u32x4 v = *(const tiff_u32x4_a1 *)(run.p + (pos - run.off));
        w[0] = v.x, w[1] = v.y, w[2] = v.z, w[3] = v.w;
        if (pos + 16 == (int64_t)run.off + run.len) ++*r;
        return;
    }
#pragma unroll
    for (int b = 0; b < 16; b++) {
        if (b < cnt) {
            if (pos + b >= (int64_t)run.off + run.len) run = runs[++*r];
            w[b >> 2] |= (uint32_t)run.p[pos + b - run.off] << (8 * (b & 3));
        }
    }
    if (pos + cnt == (int64_t)run.off + run.len) ++*r;
}
__device__ __forceinline__ uint32_t exr_raw_byte(const ExrRun *__restrict__ runs, int n_runs, int64_t pos) {
    const ExrRun run = runs[exr_find_run(runs, n_runs, pos)];
    return run.p[pos - run.off];
}

__global__ __launch_bounds__(64 * kExrTilesPerWg) void zs_exr_undo_kernel(const ExrJob *__restrict__ jobs, const int32_t *__restrict__ tile_off, int n, int64_t first,
                                                                             const ExrRun *__restrict__ all_runs, const uint8_t *__restrict__ seg) {
    int j, q;
    if (!exr_my_tile(tile_off, n, first, &j, &q)) return;
    const ExrJob jb = jobs[j];
    const ExrRun *runs = all_runs + jb.run0;
    const int lane = (int)threadIdx.x & 63;
    const int64_t U = jb.len, h = (U + 1) >> 1, a = (int64_t)q * kExrSeg;
    if (jb.plain) {
        // the stored bytes are the raw bytes: the tile's 2 * kExrSeg of them, 32 a lane and pass
        for (int64_t pos = 2 * a + 32 * lane; pos < 2 * a + kExrTile && pos < U; pos += 2 * kExrPass) {
            int r = exr_find_run(runs, jb.n_runs, pos);
#pragma unroll
            for (int half = 0; half < 2; half++) {
                const int64_t at = pos + 16 * half;
                const int cnt = (int)(U - at < 16 ? U - at : 16);
                if (cnt <= 0) break;
                uint32_t w[4];
                exr_load16(jb.t, at, U, w);
                exr_scatter16(runs, &r, at, cnt, w);
            }
        }
        return;
    }
    // the carries: what the first half holds in front of a, and all of the first half plus what the second holds in front of h + a
    const int n_tiles = tile_off[j + 1] - tile_off[j];
    const uint8_t *sg = seg + 2 * (int64_t)tile_off[j];
    uint32_t c1 = 0, c2 = 0;
    for (int k = lane; k < n_tiles + q; k += 64) {
        const uint32_t s = sg[k];
        c2 += s;
        c1 += k < q ? s : 0;
    }
    c1 = tiff_wave_sum(c1), c2 = tiff_wave_sum(c2);
    const int odd = (int)(h & 1);
    for (int64_t base = a; base < a + kExrSeg && base < h; base += kExrPass) {
        const int64_t pos = base + 16 * lane;
        uint32_t wa[4], wb[4], raw[8];
        exr_load16(jb.t, pos, h, wa);
        exr_load16(jb.t + h, pos, U - h, wb);
        const uint32_t ta = exr_lane_scan(wa) & 0xFF, tb = exr_lane_scan(wb) & 0xFF;
        const uint32_t ua = tiff_wave_scan(ta, lane), ub = tiff_wave_scan(tb, lane);
        exr_lane_finish(wa, c1 + ua - ta, 0);
        exr_lane_finish(wb, c2 + ub - tb, odd);
        c1 += (uint32_t)__builtin_amdgcn_readlane((int)ua, 63), c2 += (uint32_t)__builtin_amdgcn_readlane((int)ub, 63);
        exr_interleave(wa, wb, raw);
        const int64_t out = 2 * pos;
        if (out < U) {
            int r = exr_find_run(runs, jb.n_runs, out);
#pragma unroll
            for (int half = 0; half < 2; half++) {
                const int64_t at = out + 16 * half;
                const int cnt = (int)(U - at < 16 ? U - at : 16);
                if (cnt <= 0) break;
                exr_scatter16(runs, &r, at, cnt, raw + 4 * half);
            }
        }
    }
}

__global__ __launch_bounds__(64 * kExrTilesPerWg) void zs_exr_predict_kernel(const ExrJob *__restrict__ jobs, const int32_t *__restrict__ tile_off, int n, int64_t first,
                                                                                const ExrRun *__restrict__ all_runs) {
    int j, q;
    if (!exr_my_tile(tile_off, n, first, &j, &q)) return;
    const ExrJob jb = jobs[j];
    const ExrRun *runs = all_runs + jb.run0;
    const int lane = (int)threadIdx.x & 63;
    const int64_t U = jb.len, h = (U + 1) >> 1, a = (int64_t)q * kExrSeg;
    for (int64_t base = a; base < a + kExrSeg && base < h; base += kExrPass) {
        const int64_t pos = base + 16 * lane, in = 2 * pos;
        uint32_t raw[8] = {0, 0, 0, 0, 0, 0, 0, 0}, wa[4], wb[4];
        if (in < U) {
            int r = exr_find_run(runs, jb.n_runs, in);
#pragma unroll
            for (int half = 0; half < 2; half++) {
                const int64_t at = in + 16 * half;
                const int cnt = (int)(U - at < 16 ? U - at : 16);
                if (cnt <= 0) break;
                exr_gather16(runs, &r, at, cnt, raw + 4 * half);
            }
        }
        if (jb.plain) {
            exr_store16(jb.t, in, U, raw);
            exr_store16(jb.t, in + 16, U, raw + 4);
            continue;
        }
        // the two bytes in front of the lane's 32: the neighbour's last two; the pass's first lane reads them
        uint32_t before = (uint32_t)__shfl_up((int)raw[7], 1, 64) >> 16;
        if (lane == 0) {
            if (base == 0) before = 128 | (h >= 1 && U > 1 ? exr_raw_byte(runs, jb.n_runs, 2 * (h - 1)) : 0) << 8;  // (the second half goes on from the first one's last byte)
            else before = exr_raw_byte(runs, jb.n_runs, in - 2) | exr_raw_byte(runs, jb.n_runs, in - 1) << 8;
        }
        exr_split(raw, wa, wb);
        exr_lane_diff(wa, before & 0xFF);
        exr_lane_diff(wb, before >> 8);
        exr_store16(jb.t, pos, h, wa);
        exr_store16(jb.t + h, pos, U - h, wb);
    }
}

}  // namespace zs
