// zs_png.hip -- KU: PNG scanline reconstruction on the device, the inverse of KP (zs_kernels.hip); KA, KS, KX, KG, KV, KM, KD and the crop behind it.  What inflate leaves for
// an IDAT payload is, per row, a filter-type byte and the filtered bytes; reconstruction reads reconstructed neighbours
// (left, above, above-left), so it is serial along a row and across rows.  Two kernels:
//   zs_png_scan_kernel      one workgroup per image over its type bytes: the first invalid one, and the segments
//                           (zs_png.h png_row_cuts) appended to one list for the whole batch
//   zs_png_unfilter_kernel  a fixed grid over that list, one workgroup per segment at a time, the skewed wavefront of
//                           zs_png.h inside it.  No workgroup waits for another.
#pragma once

#include <hip/hip_runtime.h>

#include "zs_png.h"

namespace zs {

struct PngImg {
    const uint8_t *in;
    uint8_t *out;
    int64_t row_bytes;
    int32_t height, bpp;
};
struct PngSeg {
    int32_t img, row0, row1, pad;
};

constexpr int kPngNoBadRow = 0x7FFFFFFF;
constexpr int kPngMaxLds = png_lds_bytes(4, png_waves(4)) > png_lds_bytes(8, png_waves(8)) ? png_lds_bytes(4, png_waves(4)) : png_lds_bytes(8, png_waves(8));

// counters[0]: segments of the batch (zeroed before the launch); counters[1 + i]: image i's first row with a type > 4
__global__ __launch_bounds__(256) void zs_png_scan_kernel(const PngImg *imgs, PngSeg *segs, int32_t *counters) {
    __shared__ int s_cnt[4], s_base, s_prev, s_bad;
    const int img = (int)blockIdx.x, tid = (int)threadIdx.x, w = tid >> 6, lane = tid & 63;
    const PngImg im = imgs[img];
    const int64_t pitch = im.row_bytes + 1;
    if (tid == 0) s_prev = -1, s_bad = kPngNoBadRow;
    __syncthreads();
    for (int64_t r0 = 0; r0 < im.height; r0 += 256) {
        const int64_t r = r0 + tid;
        const bool valid = r < im.height;
        const int ft = valid ? im.in[r * pitch] : 2;
        const bool cut = valid && (r == 0 || png_row_cuts(ft));
        if (valid && ft > 4) atomicMin(&s_bad, (int)r);
        const unsigned long long m = __ballot(cut);
        if (lane == 0) s_cnt[w] = __popcll(m);
        __syncthreads();
        const int tot = s_cnt[0] + s_cnt[1] + s_cnt[2] + s_cnt[3];
        int before = __popcll(m & ((1ull << lane) - 1));
        for (int i = 0; i < w; i++) before += s_cnt[i];
        if (tid == 0 && tot > 0) s_base = atomicAdd(&counters[0], tot);
        __syncthreads();
        if (cut) {
            const int slot = s_base + before;
            segs[slot].img = img;
            segs[slot].row0 = (int)r;
            const int prev = before > 0 ? slot - 1 : s_prev;  // the segment that ends where this one starts
            if (prev >= 0) segs[prev].row1 = (int)r;
        }
        __syncthreads();
        if (tid == 0 && tot > 0) s_prev = s_base + tot - 1;
    }
    __syncthreads();
    if (tid == 0) {
        segs[s_prev].row1 = im.height;  // (row 0 always starts a segment)
        counters[1 + img] = s_bad;
    }
}

template <int BPP>
__device__ __forceinline__ uint64_t png_lds_px(const uint8_t *p) {
    if constexpr (BPP == 8) return *(const uint64_t *)p;
    else if constexpr (BPP == 4) return *(const uint32_t *)p;
    else if constexpr (BPP == 2) return *(const uint16_t *)p;
    else {
        uint64_t v = 0;
#pragma unroll
        for (int j = 0; j < BPP; j++) v |= (uint64_t)p[j] << (8 * j);
        return v;
    }
}
template <int BPP>
__device__ __forceinline__ void png_lds_put(uint8_t *p, uint64_t v) {
    if constexpr (BPP == 8) *(uint64_t *)p = v;
    else if constexpr (BPP == 4) *(uint32_t *)p = (uint32_t)v;
    else if constexpr (BPP == 2) *(uint16_t *)p = (uint16_t)v;
    else {
#pragma unroll
        for (int j = 0; j < BPP; j++) p[j] = (uint8_t)(v >> (8 * j));
    }
}

// what lane L-1 holds, in lane L; lane 0 gets `first` (DPP wave_shr:1, nothing goes through memory)
template <int BPP>
__device__ __forceinline__ uint64_t png_from_lane_above(uint64_t v, uint64_t first) {
    const uint32_t lo = (uint32_t)__builtin_amdgcn_update_dpp((int)(uint32_t)first, (int)(uint32_t)v, 0x138, 0xf, 0xf, false);
    if constexpr (BPP <= 4) return lo;
    else {
        const uint32_t hi = (uint32_t)__builtin_amdgcn_update_dpp((int)(uint32_t)(first >> 32), (int)(uint32_t)(v >> 32), 0x138, 0xf, 0xf, false);
        return ((uint64_t)hi << 32) | lo;
    }
}

// lane `from`'s value in every lane (`from` is the same for the whole wave)
template <int BPP>
__device__ __forceinline__ uint64_t png_lane_value(uint64_t v, int from) {
    const uint32_t lo = (uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)v, from);
    if constexpr (BPP <= 4) return lo;
    else return ((uint64_t)(uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)(v >> 32), from) << 32) | lo;
}

// `rows` rows of `nbytes` bytes each, row i at g + i * gpitch (any alignment) and at l + i * lpitch (4-aligned): whole
// dwords over the 64 lanes, row after row, and the last bytes of a row one by one -- nothing outside a row is touched
template <bool TO_LDS>
__device__ __forceinline__ void png_copy_rows(uint8_t *l, int lpitch, uint8_t *g, int64_t gpitch, int rows, int nbytes, int dw_per_row, int lane) {
    const int total = rows * dw_per_row;
    if (nbytes == 4 * dw_per_row) {  // whole dwords only (all but a row's last tile column): sixteen loads on their way, then their stores
        for (int base = 0; base < total; base += 64 * 16) {
            uint32_t v[16];
#pragma unroll
            for (int j = 0; j < 16; j++) {
                if (base + 64 * j >= total) break;  // (the same for the whole wave: a band of few rows issues few loads)
                const int at = base + 64 * j + lane, idx = at < total ? at : total - 1;  // (past the end: the last dword again, not stored)
                const int i = idx / dw_per_row, off = 4 * (idx - i * dw_per_row);
                if (TO_LDS) __builtin_memcpy(&v[j], g + i * gpitch + off, 4);
                else v[j] = *(const uint32_t *)(l + i * lpitch + off);
            }
#pragma unroll
            for (int j = 0; j < 16; j++) {
                const int idx = base + 64 * j + lane;
                const int i = idx / dw_per_row, off = 4 * (idx - i * dw_per_row);
                if (idx < total) {
                    if (TO_LDS) *(uint32_t *)(l + i * lpitch + off) = v[j];
                    else __builtin_memcpy(g + i * gpitch + off, &v[j], 4);
                }
            }
        }
        return;
    }
    for (int idx = lane; idx < total; idx += 64) {
        const int i = idx / dw_per_row, off = 4 * (idx - i * dw_per_row);
        uint8_t *gp = g + i * gpitch + off, *lp = l + i * lpitch + off;
        if (off + 4 <= nbytes) {
            uint32_t v;
            if (TO_LDS) {
                __builtin_memcpy(&v, gp, 4);
                *(uint32_t *)lp = v;
            } else {
                v = *(const uint32_t *)lp;
                __builtin_memcpy(gp, &v, 4);
            }
        } else {
            for (int b = off; b < nbytes; b++) {
                if (TO_LDS) lp[b - off] = gp[b - off];
                else gp[b - off] = lp[b - off];
            }
        }
    }
}

// One segment, rows [row0, row1) of image `im`, by the `waves` waves of the workgroup (zs_png.h for the schedule).
// lds: waves x tile (64 rows of png_tile_stride(BPP) bytes), then at bnd_off waves x kPngBndBytes.
template <int BPP>
__device__ void png_segment(const PngImg &im, int row0, int row1, uint8_t *lds, int bnd_off, int waves) {
    const int w = __builtin_amdgcn_readfirstlane((int)threadIdx.x >> 6), lane = (int)threadIdx.x & 63;
    constexpr int stride = png_tile_stride(BPP), col_bytes = kPngChunk * BPP, dw_per_col = col_bytes / 4;
    uint8_t *tile = lds + w * (kPngRows * stride), *bnd = lds + bnd_off + w * kPngBndBytes;
    uint8_t *my = tile + lane * stride;
    const int64_t rb = im.row_bytes, npx = png_npx(rb, BPP), nq = png_nq(npx);
    const int64_t nbands = ((int64_t)(row1 - row0) + kPngRows - 1) / kPngRows;
    const int64_t steps = png_total_steps(nbands, waves, nq), period = png_period(nq, waves);
    int64_t k = w, q = -2 * (int64_t)w;  // this wave's band, and the chunk step of that band
    uint64_t a = 0, cprev = 0, pout = 0;
    PngSel sel = png_sel(0);
    bool rowvalid = false;
    for (int64_t T = 0; T < steps; T++) {
        const bool active = q >= 0 && q < nq && k < nbands;
        const int64_t y0 = row0 + k * kPngRows;
        const int rows = active ? (int)((int64_t)row1 - y0 < kPngRows ? (int64_t)row1 - y0 : kPngRows) : 0;
        const int slot = (int)(q & 1);
        if (active) {
            if (q == 0) {
                a = cprev = pout = 0;
                rowvalid = lane < rows;
                const int ft = rowvalid ? im.in[(y0 + lane) * (rb + 1)] : 0;
                sel = png_sel(ft);  // (a type above 4 selects nothing: None)
            }
            const int64_t byte0 = q * col_bytes;  // tile column q of the rows
            const int nbytes = (int)(rb - byte0 < col_bytes ? rb - byte0 : col_bytes);
            if (nbytes > 0) {
                png_copy_rows<true>(tile + slot * col_bytes, stride, const_cast<uint8_t *>(im.in) + y0 * (rb + 1) + 1 + byte0, rb + 1, rows, nbytes,
                                    dw_per_col, lane);
                // the row above the band: zeros above a segment, else what another wave of this workgroup stored at least two
                // chunk steps ago.  That store is visible here because of the barriers in between: __syncthreads() orders global
                // memory at workgroup scope, and the waves of a workgroup share their CU's L1.  (Not so in tgsplit mode, where a
                // workgroup may span CUs: this kernel is not built for it.)
                if (w == 0) {
                    if (k == 0) {
                        for (int i = lane; i < dw_per_col; i += 64) *(uint32_t *)(bnd + slot * col_bytes + 4 * i) = 0;
                    } else
                        png_copy_rows<true>(bnd + slot * col_bytes, 0, im.out + (y0 - 1) * rb + byte0, 0, 1, nbytes, dw_per_col, lane);
                }
            }
        }
        __syncthreads();
        if (active) {
            // the row above lane 0, tile column q: pixel s in lane s, handed to lane 0 at inner step s
            const uint64_t above = png_lds_px<BPP>(bnd + slot * col_bytes + lane * BPP);
            const int64_t x0 = q * kPngChunk - lane;
            for (int g = 0; g < kPngChunk; g += 8) {
                uint64_t f[8];
                bool act[8];
#pragma unroll
                for (int u = 0; u < 8; u++) {
                    const int64_t x = x0 + g + u;
                    act[u] = rowvalid && x >= 0 && x < npx;
                    f[u] = png_lds_px<BPP>(my + (int)(x & (kPngRing - 1)) * BPP);  // (inside the tile whatever x is)
                }
#pragma unroll
                for (int u = 0; u < 8; u++) asm volatile("" : "+v"(f[u]));  // all eight reads are on their way before the first is used
#pragma unroll
                for (int u = 0; u < 8; u++) {
                    const uint64_t b = png_from_lane_above<BPP>(pout, png_lane_value<BPP>(above, g + u));
                    const uint64_t rec = png_recon_px<BPP>(sel, act[u] ? f[u] : 0, a, b, cprev);
                    pout = act[u] ? rec : 0;
                    a = act[u] ? rec : a;
                    cprev = b;
                    if (act[u]) png_lds_put<BPP>(my + (int)((x0 + g + u) & (kPngRing - 1)) * BPP, rec);
                }
            }
        }
        if (active && q >= 1) {  // tile column q-1 is complete in every row of the band (the slot no wave reads in this chunk step)
            const int64_t byte0 = (q - 1) * col_bytes;
            const int nbytes = (int)(rb - byte0 < col_bytes ? rb - byte0 : col_bytes);
            const int pslot = slot ^ 1;
            png_copy_rows<false>(tile + pslot * col_bytes, stride, im.out + y0 * rb + byte0, rb, rows, nbytes, dw_per_col, lane);
            if (w + 1 < waves)  // its last row is the row above the next band, which is two chunk steps behind
                for (int i = lane; i < dw_per_col; i += 64)
                    *(uint32_t *)(bnd + kPngBndBytes + pslot * col_bytes + 4 * i) = *(const uint32_t *)(tile + (kPngRows - 1) * stride + pslot * col_bytes + 4 * i);
        }
        __syncthreads();  // what was stored and handed on is there for the next chunk step's loads
        if (++q == period) q = 0, k += waves;
    }
}

__global__ __launch_bounds__(256) void zs_png_unfilter_kernel(const PngImg *imgs, const PngSeg *segs, const int32_t *counters, int bnd_off) {
    extern __shared__ __attribute__((aligned(16))) uint8_t png_lds[];
    const int total = counters[0], waves = (int)blockDim.x >> 6;
    for (int item = (int)blockIdx.x; item < total; item += (int)gridDim.x) {
        const PngSeg sg = segs[item];
        const PngImg im = imgs[sg.img];
        switch (im.bpp) {
        case 1: png_segment<1>(im, sg.row0, sg.row1, png_lds, bnd_off, waves); break;
        case 2: png_segment<2>(im, sg.row0, sg.row1, png_lds, bnd_off, waves); break;
        case 3: png_segment<3>(im, sg.row0, sg.row1, png_lds, bnd_off, waves); break;
        case 4: png_segment<4>(im, sg.row0, sg.row1, png_lds, bnd_off, waves); break;
        case 5: png_segment<5>(im, sg.row0, sg.row1, png_lds, bnd_off, waves); break;
        case 6: png_segment<6>(im, sg.row0, sg.row1, png_lds, bnd_off, waves); break;
        case 7: png_segment<7>(im, sg.row0, sg.row1, png_lds, bnd_off, waves); break;
        default: png_segment<8>(im, sg.row0, sg.row1, png_lds, bnd_off, waves); break;
        }
        __syncthreads();
    }
}

// KA: the Adam7 interleave, as a gather.  The grid is the flat list of all interlaced images' output rows (row_off as for
// KP, zs_png.h png_row_image), four rows a workgroup: wave w takes row 4 * block + w, and its lanes the row's aligned groups
// of G bytes (zs_png.h adam7_group), 64 at a time -- one full-width store per lane, contiguous over the wave.  Every pixel's
// source is computed from (x, y); the reads are plain cached loads from the two to four pass rows that feed the output
// row, each of them contiguous over the wave.  No atomics, no LDS: no output byte has two writers.
constexpr int kAdam7RowsPerWg = 4;

template <int G>
__global__ __launch_bounds__(64 * kAdam7RowsPerWg) void zs_png_adam7_kernel(const Adam7Img *imgs, const int32_t *row_off, int n, int64_t row0) {
    const int w = __builtin_amdgcn_readfirstlane((int)threadIdx.x >> 6), lane = (int)threadIdx.x & 63;
    const int64_t r = row0 + (int64_t)blockIdx.x * kAdam7RowsPerWg + w;
    if (r >= (int64_t)row_off[n]) return;
    const int i = png_row_image(row_off, n, r);
    const Adam7Img &im = imgs[i];  // (left in memory: off[] is indexed by a pass that differs from lane to lane)
    const int64_t y = r - row_off[i], rb = png_bits_row_bytes(im.width, im.bits);
    uint8_t *dst = im.out + y * rb;
    const uint64_t addr = (uint64_t)(uintptr_t)dst;
    if (im.bits < 8) {
        const int64_t ng = adam7_row_groups(addr, rb, kAdam7GroupBits), b0 = adam7_row_b0(addr, kAdam7GroupBits);
        for (int64_t g = lane; g < ng; g += 64) adam7_group<kAdam7GroupBits>(im, y, rb, dst, b0 + g * kAdam7GroupBits);
    } else {
        const int64_t ng = adam7_row_groups(addr, rb, G), b0 = adam7_row_b0(addr, G);
        for (int64_t g = lane; g < ng; g += 64) adam7_group<G>(im, y, rb, dst, b0 + g * G);
    }
}

// KS: the Adam7 split, KA's inverse and shaped like it.  The grid is the flat list of all images' pass rows (absent passes
// have none), four a workgroup: wave w takes pass row 4 * block + w, finds its image (png_row_image), its pass and its row in
// the pass (all uniform over the wave), and its lanes take the pass row's aligned groups of G bytes (zs_png.h
// adam7_split_group), 64 at a time -- one full-width store per lane, contiguous over the wave.  The reads are plain cached
// loads from the one source row, at a stride of 1, 2, 4 or 8 pixels.  No atomics, no LDS: no output byte has two writers.
constexpr int kSplitRowsPerWg = 4;

template <int G>
__global__ __launch_bounds__(64 * kSplitRowsPerWg) void zs_png_split_kernel(const Adam7SplitImg *imgs, const int32_t *row_off, int n, int64_t row0) {
    const int w = __builtin_amdgcn_readfirstlane((int)threadIdx.x >> 6), lane = (int)threadIdx.x & 63;
    const int64_t r = row0 + (int64_t)blockIdx.x * kSplitRowsPerWg + w;
    if (r >= (int64_t)row_off[n]) return;
    const int i = png_row_image(row_off, n, r);
    const Adam7SplitImg &im = imgs[i];
    const int64_t local = r - row_off[i];
    const int p = adam7_split_pass(im, local);
    const int64_t j = local - im.row0[p], prb = png_bits_row_bytes(adam7_pass_width(im.width, p), im.bits);
    uint8_t *dst = im.passes + im.off[p] + j * prb;
    const uint64_t addr = (uint64_t)(uintptr_t)dst;
    if (im.bits < 8 && p != 6) {
        const int64_t ng = adam7_row_groups(addr, prb, kAdam7GroupBits), b0 = adam7_row_b0(addr, kAdam7GroupBits);
        for (int64_t g = lane; g < ng; g += 64) adam7_split_group<kAdam7GroupBits>(im, p, j, prb, dst, b0 + g * kAdam7GroupBits);
    } else {
        const int64_t ng = adam7_row_groups(addr, prb, G), b0 = adam7_row_b0(addr, G);
        for (int64_t g = lane; g < ng; g += 64) adam7_split_group<G>(im, p, j, prb, dst, b0 + g * G);
    }
}

// KX: raw scanlines to RGBA8 / RGBA16 (zs_png.h png_expand_group), shaped like KA.  The grid is the flat list of all images'
// output rows, four rows a workgroup: wave w takes row 4 * block + w, and its lanes the row's address-aligned groups of 16
// bytes, 64 at a time -- one full-width store per lane, 1 KiB contiguous over the wave; the ragged first and last groups of
// a row go out pixel by pixel.  A lane reads the input bytes that hold its 4 (RGBA16: 2) pixels with plain cached loads,
// contiguous over the wave as well (at 1, 2 and 4 bits neighbouring lanes share bytes).  The wave of a palette row first
// copies its image's table (1 KiB) into an LDS slice of its own.  No atomics, no traffic between waves: no output byte has
// two writers.
constexpr int kExpandRowsPerWg = 4;

template <int F>
__global__ __launch_bounds__(64 * kExpandRowsPerWg) void zs_png_expand_kernel(const PngExpandImg *imgs, const int32_t *row_off, const uint32_t *tables, int n,
                                                                               int64_t row0) {
    __shared__ uint32_t s_pal[kExpandRowsPerWg][kPngPalEntries];
    const int w = __builtin_amdgcn_readfirstlane((int)threadIdx.x >> 6), lane = (int)threadIdx.x & 63;
    const int64_t r = row0 + (int64_t)blockIdx.x * kExpandRowsPerWg + w;
    const bool active = r < (int64_t)row_off[n];
    const int i = active ? png_row_image(row_off, n, r) : 0;
    const PngExpandImg im = imgs[i];
    if (active && im.color == 3)
        for (int k = lane; k < kPngPalEntries; k += 64) s_pal[w][k] = tables[(int64_t)im.pal_off + k];
    __syncthreads();  // (every wave arrives: none has left yet)
    if (!active) return;
    const int64_t y = r - row_off[i], rb = (int64_t)im.width * png_expand_bytes(F);
    uint8_t *dst = im.out + y * rb;
    const uint64_t addr = (uint64_t)(uintptr_t)dst;
    const int64_t ng = adam7_row_groups(addr, rb, kPngExpandGroup), b0 = adam7_row_b0(addr, kPngExpandGroup);
    for (int64_t g = lane; g < ng; g += 64) png_expand_group<F>(im, s_pal[w], y, dst, b0 + g * kPngExpandGroup);
}

// KG: RGBA8 / RGBA16 to raw scanlines (zs_png.h png_pack_group), KX's inverse and shaped like it.  The grid is the flat list of
// all images' output rows, four rows a workgroup: wave w takes row 4 * block + w, and its lanes the row's address-aligned
// groups of 16 output bytes (4 at 1, 2 and 4 bits a pixel, where 16 bytes would be up to 128 source pixels a lane), 64 at a
// time -- one full-width store per lane, contiguous over the wave; the ragged first and last groups of a row go out byte by
// byte.  The source pixels are aligned loads of 4 or 8 bytes, contiguous over the wave.  The wave of a palette row first
// copies its image's lookup table (2 KiB) into an LDS slice of its own; the pixels that find no entry are counted per lane,
// summed over the wave, and added once per wave to the image's word of `unmatched` (zeroed by the host).  No other atomics,
// no traffic between waves: no output byte has two writers.
constexpr int kPackRowsPerWg = 4;

template <int F>
__global__ __launch_bounds__(64 * kPackRowsPerWg) void zs_png_pack_kernel(const PngPackImg *imgs, const int32_t *row_off, const uint32_t *tables,
                                                                          unsigned long long *unmatched, int n, int64_t row0) {
    __shared__ uint32_t s_tab[kPackRowsPerWg][kPngPackTableWords];
    const int w = __builtin_amdgcn_readfirstlane((int)threadIdx.x >> 6), lane = (int)threadIdx.x & 63;
    const int64_t r = row0 + (int64_t)blockIdx.x * kPackRowsPerWg + w;
    const bool active = r < (int64_t)row_off[n];
    const int i = active ? png_row_image(row_off, n, r) : 0;
    const PngPackImg im = imgs[i];
    if (active && im.color == 3)
        for (int k = lane; k < kPngPackTableWords; k += 64) s_tab[w][k] = tables[(int64_t)im.pal_off + k];
    __syncthreads();  // (every wave arrives: none has left yet)
    if (!active) return;
    const int bits = im.depth * (im.color == 2 ? 3 : im.color == 4 ? 2 : im.color == 6 ? 4 : 1), G = png_pack_group_bytes(bits);
    const int64_t y = r - row_off[i], rb = png_bits_row_bytes(im.width, bits);
    uint8_t *dst = im.out + y * rb;
    const uint64_t addr = (uint64_t)(uintptr_t)dst;
    const int64_t ng = adam7_row_groups(addr, rb, G), b0 = adam7_row_b0(addr, G);
    uint32_t miss = 0;
    for (int64_t g = lane; g < ng; g += 64) miss += png_pack_group<F>(im, s_tab[w], y, rb, dst, b0 + g * G);
    if (im.color == 3) {  // (the same for the whole wave)
        for (int o = 32; o > 0; o >>= 1) miss += __shfl_xor(miss, o);
        if (lane == 0 && miss) atomicAdd(&unmatched[i], (unsigned long long)miss);
    }
}

// KV: the survey.  Two launches.  The first runs over the flat list of (image, kSurveyRows rows of it) items, one workgroup
// an item: the item's pixels are one contiguous run, taken in address-aligned groups of 16 bytes (the ragged ends pixel by
// pixel).  Every lane ORs its pixels' violation bits (zs_png.h png_survey_pixel), the workgroup ORs the lanes' through LDS;
// low8 pixels go into a set of the workgroup in LDS -- open addressing, atomicCAS on the slot, a counter behind it -- unless
// they equal the pixel in front of them in the lane's group, and until the counter passes 256.  The workgroup then writes its
// record (mask, count, colours) to its own slot.  The second launch merges an image's records with one workgroup through the
// same set.  No atomics outside LDS, no byte with two writers; the order of a record's colours depends on the run, their set
// and count do not, and the host sorts them.
__device__ __forceinline__ void png_survey_insert(uint32_t *slots, int *count, uint32_t c) {
    if (*(volatile int *)count > 256) return;  // (257 are enough to know)
    uint32_t h = png_color_hash(c, 10);
    for (int t = 0; t < kSurveySlots; t++) {
        uint32_t cur = ((volatile uint32_t *)slots)[h];
        if (cur == kSurveyEmpty) {
            cur = atomicCAS(&slots[h], kSurveyEmpty, c);
            if (cur == kSurveyEmpty) {
                atomicAdd(count, 1);
                return;
            }
        }
        if (cur == c) return;
        h = (h + 1) & (kSurveySlots - 1);
    }
}

// the workgroup's set and mask -> *rec (every thread calls; s_pos is zero on entry)
__device__ __forceinline__ void png_survey_emit(const uint32_t *slots, const int *count, int *s_pos, uint32_t mask, PngSurveyRec *rec) {
    const int tid = (int)threadIdx.x;
    const int cnt = *count;
    if (cnt <= 256)
        for (int k = tid; k < kSurveySlots; k += 256) {
            const uint32_t c = slots[k];
            if (c != kSurveyEmpty) rec->colors[atomicAdd(s_pos, 1)] = c;  // (cnt slots are taken: the positions stay below 256)
        }
    if (tid == 0) rec->mask = mask, rec->count = cnt <= 256 ? (uint32_t)cnt : kSurveyMany;
}

template <int F>
__global__ __launch_bounds__(256) void zs_png_survey_kernel(const PngSurveyImg *imgs, const int32_t *item_off, int n, PngSurveyRec *recs) {
    __shared__ uint32_t s_slots[kSurveySlots];
    __shared__ int s_count, s_pos;
    __shared__ uint32_t s_mask;
    constexpr int P = png_expand_bytes(F), N = 16 / P;
    const int tid = (int)threadIdx.x;
    const int64_t item = (int64_t)blockIdx.x;
    const int i = png_row_image(item_off, n, item);
    const PngSurveyImg im = imgs[i];
    for (int k = tid; k < kSurveySlots; k += 256) s_slots[k] = kSurveyEmpty;
    if (tid == 0) s_count = 0, s_pos = 0, s_mask = 0;
    __syncthreads();
    const int64_t y0 = (item - item_off[i]) * kSurveyRows, y1 = y0 + kSurveyRows < im.height ? y0 + kSurveyRows : im.height;
    const uint8_t *p = im.in + y0 * im.row_pixels * P;
    const int64_t nb = (y1 - y0) * im.row_pixels * P;  // the item's bytes
    int64_t head = (int64_t)((16 - ((uint64_t)(uintptr_t)p & 15)) & 15);  // bytes in front of the first aligned group (whole pixels: p is P-aligned)
    if (head > nb) head = nb;
    const int64_t groups = (nb - head) >> 4, tail = nb - head - (groups << 4);
    uint32_t mask = 0;
    auto take = [&](uint64_t raw, bool have_prev, uint64_t prev) {
        uint32_t c;
        const uint32_t m = png_survey_pixel<F>(raw, &c);
        mask |= m;
        if (m & kSvNotLow8) return;  // (the image's colours are not asked for)
        if (c == kSurveyEmpty) mask |= kSvWhite;
        else if (!(have_prev && raw == prev)) png_survey_insert(s_slots, &s_count, c);
    };
    for (int64_t g = tid; g < groups; g += 256) {
        uint64_t v[2];
        __builtin_memcpy(v, __builtin_assume_aligned(p + head + (g << 4), 16), 16);
        if constexpr (N == 4) {
            const uint64_t px[4] = {v[0] & 0xFFFFFFFFu, v[0] >> 32, v[1] & 0xFFFFFFFFu, v[1] >> 32};
#pragma unroll
            for (int j = 0; j < 4; j++) take(px[j], j > 0, j > 0 ? px[j - 1] : 0);
        } else {
            take(v[0], false, 0);
            take(v[1], true, v[0]);
        }
    }
    {  // the ragged ends: fewer than 2 * N pixels, one a thread
        const int64_t nh = head / P, nt = tail / P;
        if (tid < nh + nt) {
            const uint8_t *q = tid < nh ? p + (int64_t)tid * P : p + head + (groups << 4) + ((int64_t)tid - nh) * P;
            uint64_t raw = 0;
            __builtin_memcpy(&raw, __builtin_assume_aligned(q, P), P);
            take(raw, false, 0);
        }
    }
    if (mask) atomicOr(&s_mask, mask);
    __syncthreads();
    png_survey_emit(s_slots, &s_count, &s_pos, s_mask, &recs[item]);
}

// one workgroup an image: its items' records -> the image's record
__global__ __launch_bounds__(256) void zs_png_survey_merge_kernel(const int32_t *item_off, const PngSurveyRec *recs, PngSurveyRec *out) {
    __shared__ uint32_t s_slots[kSurveySlots];
    __shared__ int s_count, s_pos;
    __shared__ uint32_t s_mask;
    const int tid = (int)threadIdx.x, i = (int)blockIdx.x;
    for (int k = tid; k < kSurveySlots; k += 256) s_slots[k] = kSurveyEmpty;
    if (tid == 0) s_count = 0, s_pos = 0, s_mask = 0;
    __syncthreads();
    const int64_t r0 = item_off[i], r1 = item_off[i + 1];
    uint32_t mask = 0;
    for (int64_t k = r0 * 256 + tid; k < r1 * 256; k += 256) {  // record k >> 8 (the same for the workgroup), colour tid of it
        const PngSurveyRec &rc = recs[k >> 8];
        if (tid == 0) mask |= rc.mask;
        if (rc.count == kSurveyMany) {
            if (tid == 0) atomicAdd(&s_count, (int)kSurveyMany);  // (past 256 for good)
        } else if ((uint32_t)tid < rc.count)
            png_survey_insert(s_slots, &s_count, rc.colors[tid]);
    }
    if (mask) atomicOr(&s_mask, mask);
    __syncthreads();
    png_survey_emit(s_slots, &s_count, &s_pos, s_mask, &out[i]);
}

// KM: the frames of animations composed into canvases (zs_png.h png_compose_group), one launch a call, shaped like KX.  The
// grid is the flat list of all animations' canvas rows, every row cut into stretches of 64 groups (256 pixels of RGBA8, 128
// of RGBA16: png_compose_row_waves), a wave per stretch and four waves a workgroup: a lane takes four (RGBA16: two) pixels of
// the row.  A lane carries its pixels through frames 0 .. F-1 in registers -- the current value and the value PREVIOUS puts
// back -- reads a frame's pixels only inside the frame's region (the row test is uniform over the wave; the frame's
// descriptor is indexed by the uniform frame number and comes through scalar loads) and stores its pixels into every canvas
// once: 16 bytes where the address in that canvas is 16-aligned, pixel by pixel elsewhere.  The canvases are never read.  No
// atomics, no LDS, no traffic between waves: no output byte has two writers.  (A wave per whole row, looping over the
// stretches, left one 1024 x 1024 animation with one wave per SIMD and every frame's load latency in the open: DESIGN.md.)
constexpr int kComposeWavesPerWg = 4;

template <int F>
__global__ __launch_bounds__(64 * kComposeWavesPerWg) void zs_png_compose_kernel(const PngComposeAnim *__restrict__ anims, const int32_t *__restrict__ wave_off,
                                                                                 const PngComposeFrame *__restrict__ frames, int n, int64_t wave0) {
    const int w = __builtin_amdgcn_readfirstlane((int)threadIdx.x >> 6), lane = (int)threadIdx.x & 63;
    const int64_t t = wave0 + (int64_t)blockIdx.x * kComposeWavesPerWg + w;
    if (t >= (int64_t)wave_off[n]) return;
    const int i = __builtin_amdgcn_readfirstlane(png_row_image(wave_off, n, t));  // (the same in every lane: the descriptors come through scalar loads)
    const PngComposeAnim a = anims[i];
    constexpr int N = kPngComposeGroup / png_expand_bytes(F);
    const uint32_t local = (uint32_t)(t - wave_off[i]), per_row = (uint32_t)png_compose_row_waves(a.width, F);
    const int64_t y = local / per_row, g = (int64_t)(local % per_row) * 64 + lane;
    if (g * N < a.width) png_compose_group<F>(a, frames, y, g * N);
}

// KD: the frame diff (zs_png.h png_diff_*), KM's counterpart on the way out and on KM's grid: the flat list of all
// animations' canvas rows, every row cut into stretches of 64 groups of 16 bytes, a wave per stretch, four waves a
// workgroup.  A lane carries its group through canvases 0 .. F-1 in registers: it loads canvas f's group -- the load of
// canvas f + 1 is issued before canvas f is compared -- and compares it with canvas f - 1's, so every canvas is read once.
// Per frame the wave's answer is a __ballot of "my group differs": the first and the last set lane hand over their first and
// last differing pixel (readlane: the lane numbers are uniform), and lane 0 stores the wave's record into the wave's own slot
// of the frame.  The frame loop's trip count is uniform over the wave, and every lane stays in it: a lane beyond the row
// loads nothing and never differs.  No atomics, no LDS, no traffic between waves: no record has two writers.  An animation of
// one frame has no waves in the list.
constexpr int kDiffWavesPerWg = 4;

template <int F>
__global__ __launch_bounds__(64 * kDiffWavesPerWg) void zs_png_diff_kernel(const PngDiffAnim *__restrict__ anims, const int32_t *__restrict__ wave_off, int n,
                                                                           int64_t wave0, PngDiffRec *__restrict__ recs) {
    const int w = __builtin_amdgcn_readfirstlane((int)threadIdx.x >> 6), lane = (int)threadIdx.x & 63;
    const int64_t t = wave0 + (int64_t)blockIdx.x * kDiffWavesPerWg + w;
    if (t >= (int64_t)wave_off[n]) return;
    const int i = __builtin_amdgcn_readfirstlane(png_row_image(wave_off, n, t));
    const PngDiffAnim a = anims[i];
    constexpr int P = png_expand_bytes(F), N = kPngComposeGroup / P;
    const uint32_t local = (uint32_t)(t - wave_off[i]), per_row = (uint32_t)png_compose_row_waves(a.width, F);
    const int64_t y = local / per_row, g0 = (int64_t)(local % per_row) * 64, x0 = (g0 + lane) * N;
    const int64_t rb = (int64_t)a.width * P, canvas = rb * a.height, waves = (int64_t)a.height * per_row;
    const bool mine = x0 < a.width;
    const uint8_t *p = a.in + y * rb + x0 * P;
    uint64_t prev[2] = {0, 0}, next[2] = {0, 0};
    if (mine) {
        png_diff_load<F>(p, x0, a.width, prev);
        png_diff_load<F>(p + canvas, x0, a.width, next);  // (the list holds animations of two frames and more only)
    }
    PngDiffRec *out = recs + a.rec0 + local;
    for (int f = 1; f < a.n_frames; f++, out += waves) {
        const uint64_t cur[2] = {next[0], next[1]};
        if (mine && f + 1 < a.n_frames) png_diff_load<F>(p + (int64_t)(f + 1) * canvas, x0, a.width, next);
        int first = 0, last = 0;
        const bool differs = mine && png_diff_group<F>(prev, cur, &first, &last);
        prev[0] = cur[0], prev[1] = cur[1];
        const uint64_t mask = __ballot(differs);
        PngDiffRec rec = png_diff_none();
        if (mask) {  // (uniform)
            const int lo = png_diff_first_lane(mask), hi = png_diff_last_lane(mask);
            rec = png_diff_record(lo, hi, g0, N, __builtin_amdgcn_readlane(first, lo), __builtin_amdgcn_readlane(last, hi));
        }
        if (lane == 0) *out = rec;
    }
}

// ... its second launch: one workgroup per (animation, frame >= 1) folds the frame's records, one per wave of the first
// launch, into the frame's rectangle.  Minima and maxima only: the result does not depend on the order.
__global__ __launch_bounds__(256) void zs_png_diff_merge_kernel(const PngDiffAnim *__restrict__ anims, const int32_t *__restrict__ pair_off, int n, int format,
                                                                const PngDiffRec *__restrict__ recs, PngDiffRect *__restrict__ rects) {
    __shared__ PngDiffRect s_part[4];
    const int tid = (int)threadIdx.x, lane = tid & 63, w = tid >> 6;
    const int64_t pair = (int64_t)blockIdx.x;
    const int i = png_row_image(pair_off, n, pair);
    const PngDiffAnim a = anims[i];
    const int64_t per_row = png_compose_row_waves(a.width, format), waves = (int64_t)a.height * per_row;
    const PngDiffRec *base = recs + a.rec0 + (pair - pair_off[i]) * waves;
    PngDiffRect r = png_diff_empty();
    for (int64_t k = tid; k < waves; k += 256) r = png_diff_merge(r, base[k], (int32_t)(k / per_row));
    for (int o = 32; o > 0; o >>= 1) r = png_diff_union(r, PngDiffRect{__shfl_xor(r.x0, o), __shfl_xor(r.y0, o), __shfl_xor(r.x1, o), __shfl_xor(r.y1, o)});
    if (lane == 0) s_part[w] = r;
    __syncthreads();
    if (tid == 0) rects[pair] = png_diff_union(png_diff_union(s_part[0], s_part[1]), png_diff_union(s_part[2], s_part[3]));
}

// The crop (zs_png.h png_crop_group): rectangles of images as tight rows, shaped like KX.  The grid is the flat list of all
// output rows, four rows a workgroup: wave w takes row 4 * block + w, and its lanes the row's address-aligned groups of 16
// output bytes, 64 at a time -- one full-width store per lane, contiguous over the wave, fed by one 16-byte load where source
// and destination agree modulo 16 and by pixel loads elsewhere.  No atomics, no LDS: no output byte has two writers.
constexpr int kCropRowsPerWg = 4;

template <int P>
__global__ __launch_bounds__(64 * kCropRowsPerWg) void zs_png_crop_kernel(const PngCropImg *__restrict__ imgs, const int32_t *__restrict__ row_off, int n, int64_t row0) {
    const int w = __builtin_amdgcn_readfirstlane((int)threadIdx.x >> 6), lane = (int)threadIdx.x & 63;
    const int64_t r = row0 + (int64_t)blockIdx.x * kCropRowsPerWg + w;
    if (r >= (int64_t)row_off[n]) return;
    const int i = __builtin_amdgcn_readfirstlane(png_row_image(row_off, n, r));
    const PngCropImg im = imgs[i];
    const int64_t y = r - row_off[i], rb = (int64_t)im.width * P;
    uint8_t *dst = im.out + y * rb;
    const uint64_t addr = (uint64_t)(uintptr_t)dst;
    const int64_t ng = adam7_row_groups(addr, rb, 16), b0 = adam7_row_b0(addr, 16);
    for (int64_t g = lane; g < ng; g += 64) png_crop_group<P>(im, y, rb, dst, b0 + g * 16);
}

}  // namespace zs
