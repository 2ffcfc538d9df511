// zs_crc32.hip -- KC: CRC-32 of many spans of any length and alignment in one launch, optionally copying every span to
// another place of any alignment (the framing of PNG chunks, the gather of IDAT data); and its finishing launch.
//
// Every span is cut into tiles of kCrcTile bytes; the tiles of all spans form one flat list and every wave takes tiles
// from it, kCrcWaves consecutive ones per workgroup and pass (zs_crc32.h: the algebra and the tables).  A wave reads its
// tile in 16-byte words aligned in memory -- the bytes in front of the tile in its first word are masked to zero, which
// leaves a raw value alone -- and:
//   * kStrided: lane L folds words L, L + 64, ... into its register, which a 4-lookup table moves kCrcStride bytes on
//     between two words; 16 more lookups give the word's own raw value;
//   * !kStrided: the words go through LDS and lane L owns words 8L .. 8L + 7, slice-by-16 (16 lookups a word).
// Either way lane L's register ends q_L words in front of the tile's last whole word: one multiply by x^(128 q_L) and an
// XOR across the wave give the raw value up to there, the tile's last 0..15 bytes follow one at a time.  The first tile
// of a span adds init * x^(8 * its bytes); the tile's value times x^(8 * bytes behind the tile) -- the product of the
// x^(2^k) of the set bits, multiplied up across the lanes -- is XORed into the span's word by a vector atomic.
// The copy builds every 16-byte word aligned at the destination from two neighbouring source words (the lane below's, or
// the last lane's of the pass before) and stores it whole; words that reach over the tile's ends are stored byte by byte.
#pragma once

#include <hip/hip_runtime.h>

#include "zs_crc32.h"

namespace zs {

constexpr int kCrcLdsTabWords = 20 * 256;                      // the slice and shift tables
constexpr int kCrcStageWords = (kCrcTile / 16 + kCrcTile / 128 + 2) * 4;  // a wave's tile in LDS, 16 bytes of padding per 128

__device__ __forceinline__ uint32_t crc_raw16(const uint32_t *tab, uint4 w) {
    uint32_t r;
    r = tab[15 * 256 + (w.x & 255)] ^ tab[14 * 256 + ((w.x >> 8) & 255)] ^ tab[13 * 256 + ((w.x >> 16) & 255)] ^ tab[12 * 256 + (w.x >> 24)];
    r ^= tab[11 * 256 + (w.y & 255)] ^ tab[10 * 256 + ((w.y >> 8) & 255)] ^ tab[9 * 256 + ((w.y >> 16) & 255)] ^ tab[8 * 256 + (w.y >> 24)];
    r ^= tab[7 * 256 + (w.z & 255)] ^ tab[6 * 256 + ((w.z >> 8) & 255)] ^ tab[5 * 256 + ((w.z >> 16) & 255)] ^ tab[4 * 256 + (w.z >> 24)];
    r ^= tab[3 * 256 + (w.w & 255)] ^ tab[2 * 256 + ((w.w >> 8) & 255)] ^ tab[1 * 256 + ((w.w >> 16) & 255)] ^ tab[w.w >> 24];
    return r;
}
__device__ __forceinline__ uint32_t crc_shift_stride(const uint32_t *tab, uint32_t c) {
    const uint32_t *s = tab + kCrcTabShift;
    return s[c & 255] ^ s[256 + ((c >> 8) & 255)] ^ s[512 + ((c >> 16) & 255)] ^ s[768 + (c >> 24)];
}
__device__ __forceinline__ uint32_t crc_wave_xor(uint32_t v) {
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) v ^= __shfl_xor(v, d, 64);
    return v;
}
__device__ __forceinline__ uint32_t crc_word_byte(const uint4 &w, int i) {
    const uint32_t d = i < 4 ? w.x : i < 8 ? w.y : i < 12 ? w.z : w.w;
    return (d >> (8 * (i & 3))) & 255;
}

// bytes [16m - sh, 16m - sh + 16) of the source, from source words m - 1 (`p`) and m (`c`); sh uniform in the wave
__device__ __forceinline__ uint4 crc_align_words(uint4 p, uint4 c, int sh) {
    const int start = 16 - sh, bs = (start & 3) * 8;  // the word begins `start` bytes into p
    uint32_t e0, e1, e2, e3, e4;
    switch (start >> 2) {
    case 0: e0 = p.x, e1 = p.y, e2 = p.z, e3 = p.w, e4 = c.x; break;
    case 1: e0 = p.y, e1 = p.z, e2 = p.w, e3 = c.x, e4 = c.y; break;
    case 2: e0 = p.z, e1 = p.w, e2 = c.x, e3 = c.y, e4 = c.z; break;
    case 3: e0 = p.w, e1 = c.x, e2 = c.y, e3 = c.z, e4 = c.w; break;
    default: e0 = c.x, e1 = c.y, e2 = c.z, e3 = c.w, e4 = 0; break;
    }
    return make_uint4(__funnelshift_r(e0, e1, bs), __funnelshift_r(e1, e2, bs), __funnelshift_r(e2, e3, bs), __funnelshift_r(e3, e4, bs));
}

template <bool kStrided>
__global__ __launch_bounds__(64 * kCrcWaves) void zs_crc32_tile_kernel(const Crc32Span *__restrict__ spans, const uint32_t *__restrict__ tile_off, int n_spans,
                                                                      uint32_t n_tiles, const uint32_t *__restrict__ gtab, uint32_t *__restrict__ res) {
    __shared__ uint32_t tab[kCrcLdsTabWords];
    __shared__ uint32_t stage[kStrided ? 4 : kCrcWaves * kCrcStageWords];
    for (int i = threadIdx.x; i < kCrcLdsTabWords / 4; i += blockDim.x) ((uint4 *)tab)[i] = ((const uint4 *)gtab)[i];
    __syncthreads();
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    for (uint64_t t64 = (uint64_t)blockIdx.x * kCrcWaves + wave; t64 < n_tiles; t64 += (uint64_t)gridDim.x * kCrcWaves) {
        const uint32_t t = (uint32_t)t64;
        const int si = crc32_tile_span(tile_off, n_spans, t);
        const Crc32Span sp = spans[si];
        const int64_t t0 = (int64_t)(t - tile_off[si]) * kCrcTile;              // the tile's first byte in the span
        const int len = (int)(sp.len - t0 < kCrcTile ? sp.len - t0 : kCrcTile);  // 1 .. kCrcTile
        const uintptr_t a0 = (uintptr_t)sp.src + (uintptr_t)t0;
        const int h = (int)(a0 & 15);  // the tile begins h bytes into its first word
        const uint4 *src = (const uint4 *)(a0 - (uintptr_t)h);
        const int end = h + len;       // source-relative position p: byte p of the words; the tile is [h, end)
        const int NF = end >> 4, r = end & 15, NS = (end + 15) >> 4;  // whole words, bytes of the last one, words touched
        // ---- the copy's geometry: byte p goes to address dp + p
        const bool copy = sp.dst != nullptr;
        const int skip = t0 == 0 ? (int)sp.skip : 0;
        const int vlo = h + skip < end ? h + skip : end;  // bytes [vlo, end) are copied
        const uintptr_t dp = (uintptr_t)sp.dst + (uintptr_t)t0 - (uintptr_t)sp.skip - (uintptr_t)h;
        const int sh = (int)(dp & 15);
        uint8_t *dbase = (uint8_t *)(dp - (uintptr_t)sh);       // destination word m is dbase + 16 m and holds p in [16 m - sh, 16 m - sh + 16)
        const int ND = copy && vlo < end ? (end + sh + 15) >> 4 : 0;
        const int n_pass = ((ND > NS ? ND : NS) + 63) >> 6;
        uint32_t acc = 0;
        uint4 carry = make_uint4(0, 0, 0, 0);
        uint32_t *my_stage = stage + (kStrided ? 0 : wave * kCrcStageWords);
        for (int k = 0; k < n_pass; k++) {
            const int m = k * 64 + lane;
            uint4 w = make_uint4(0, 0, 0, 0);
            if (m < NS) w = src[m];
            if (ND) {  // (uniform)
                uint4 p;
                p.x = __shfl_up(w.x, 1, 64), p.y = __shfl_up(w.y, 1, 64), p.z = __shfl_up(w.z, 1, 64), p.w = __shfl_up(w.w, 1, 64);
                if (lane == 0) p = carry;
                carry.x = __shfl(w.x, 63, 64), carry.y = __shfl(w.y, 63, 64), carry.z = __shfl(w.z, 63, 64), carry.w = __shfl(w.w, 63, 64);
                if (m < ND) {
                    const uint4 o = crc_align_words(p, w, sh);
                    const int p0 = 16 * m - sh;
                    if (p0 >= vlo && p0 + 16 <= end) *(uint4 *)(dbase + 16 * (size_t)m) = o;
                    else
                        for (int i = 0; i < 16; i++)
                            if (p0 + i >= vlo && p0 + i < end) dbase[16 * (size_t)m + i] = (uint8_t)crc_word_byte(o, i);
                }
            }
            if (m == 0 && h) {  // the bytes in front of the tile: zero
                const uint32_t keep = 0xFFFFFFFFu << (8 * (h & 3));
                const int hd = h >> 2;
                w.x = hd > 0 ? 0 : w.x & keep;
                w.y = hd > 1 ? 0 : hd == 1 ? w.y & keep : w.y;
                w.z = hd > 2 ? 0 : hd == 2 ? w.z & keep : w.z;
                w.w = hd == 3 ? w.w & keep : w.w;
            }
            if (kStrided) {
                if (m < NF) acc = crc_shift_stride(tab, acc) ^ crc_raw16(tab, w);
            } else if (m < NF) {
                *(uint4 *)(my_stage + 4 * (m + (m >> 3))) = w;
            }
        }
        int e;  // words of the tile in front of the end of the lane's register
        if (kStrided) {
            const int cnt = lane < NF ? (NF - lane + 63) >> 6 : 0;
            e = cnt ? lane + 64 * (cnt - 1) + 1 : NF;
        } else {
            __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
            __builtin_amdgcn_wave_barrier();
            __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
            const int m0 = lane * 8, m1 = m0 + 8 < NF ? m0 + 8 : NF;
            for (int m = m0; m < m1; m++) {
                uint4 w = *(const uint4 *)(my_stage + 4 * (m + (m >> 3)));
                w.x ^= acc;
                acc = crc_raw16(tab, w);
            }
            e = m0 < NF ? m1 : NF;
            __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
            __builtin_amdgcn_wave_barrier();  // (the next tile's words come into the same place)
        }
        uint32_t v = crc_wave_xor(crc32_mul(acc, gtab[kCrcTabPow128 + (NF - e)]));
        if (r) {  // the last 1..15 bytes: word NF, from byte max(h, 16 NF) - 16 NF on
            const uint4 w = src[NF];
            for (int i = NF ? 0 : h; i < r; i++) v = tab[(v ^ crc_word_byte(w, i)) & 255] ^ (v >> 8);
        }
        if (t0 == 0 && sp.init) v ^= crc32_mul(crc32_mul(sp.init, gtab[kCrcTabPow128 + (len >> 4)]), gtab[kCrcTabPow8 + (len & 15)]);
        const uint32_t after = (uint32_t)(sp.len - t0 - len);  // bytes of the span behind the tile (< 2^31)
        if (after) {
            uint32_t f = lane < 32 && ((after >> lane) & 1) ? gtab[kCrcTabX2n + ((lane + 3) & 31)] : kCrc32One;
#pragma unroll
            for (int d = 1; d <= 16; d <<= 1) f = crc32_mul(f, __shfl_xor(f, d, 64));
            v = crc32_mul(v, f);
        }
        if (lane == 0) atomicXor(res + si, v);
    }
}

// One thread per span: the CRC (the register's complement; a span without bytes never met a tile: its register is init),
// and for a framed span the twelve bytes around its data (sixteen with a prefix: zs_crc32.h png_close_chunk).
__global__ void zs_crc32_finish_kernel(const Crc32Span *__restrict__ spans, int n_spans, const uint32_t *__restrict__ res, uint32_t *__restrict__ out) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n_spans) return;
    const Crc32Span sp = spans[i];
    const uint32_t crc = ~(sp.len > 0 ? res[i] : sp.init);
    out[i] = crc;
    if (sp.frame) png_close_chunk(sp.frame, (uint32_t)(sp.len - sp.skip), sp.type, sp.has_prefix != 0, sp.prefix, crc);
}

}  // namespace zs
