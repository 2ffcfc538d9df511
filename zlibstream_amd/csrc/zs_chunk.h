// zs_chunk.h -- chunked N-dimensional arrays as HDF5 / NetCDF-4 and Zarr v2 store them (shuffle in front of deflate, chunk by
// chunk) as far as this library reads and writes them: the geometry of the chunk grid, the decomposition of a launch's flat
// item index into (chunk, row, stretch), and the per-lane step of the KN kernels (zs_chunk.hip); zs_chunk_host.inc builds the
// calls on them, tests/cpp/test_chunk_rows.cpp runs them on the host.  include/zsgpu.h states the rules in full.
//
// A chunk holds E = prod(chunk[d]) elements in C order, edge chunks padded to full size.  Shuffled, byte j of element e lies
// at j * E + e (H5Zshuffle, numcodecs Shuffle): elem_size planes of E bytes.  A row is a run along the last axis: chunk[rank-1]
// elements in the chunk, clipped to shape[rank-1] in the array, contiguous in both.  A row is cut into stretches of
// 256 * unit elements, a wave's work: four passes of 64 lanes x `unit` elements (16, 4 or 1 by the length of a row, so that a
// short row is still many lanes' work).
// Behind KN's steps: the rules of zs_chunk_filters, Fletcher-32 in closed form with its per-lane step and combine rule, and the
// per-lane steps of the delta filter; tests/cpp/test_chunk_filters.cpp runs those on the host.
#pragma once

#include <cstdint>
#include <cstring>

#include "zs_core.h"

namespace zs {

constexpr int kChunkMaxRank = 8, kChunkMaxElem = 16;
constexpr int64_t kChunkMaxBytes = 0x7FFFFFFF - 1024;  // a chunk, in one call of the engine
constexpr int kChunkPasses = 4;                        // passes of the wave over a stretch

enum { kChunkStored = 1, kChunkUnshuffled = 2, kChunkSkip = 4, kChunkAbsent = 8 };  // ZS_CHUNK_*
// a job's bytes are not shuffled; it has none: its region is `fill`; its elements (of 2, 4 or 8 bytes) lie big-endian in the chunk
enum { kJobPlain = 1, kJobFill = 2, kJobSwap = 4 };

struct ChunkGrid {  // zs_chunk_grid
    int32_t rank, elem_size;
    int64_t shape[kChunkMaxRank], chunk[kChunkMaxRank];
    int32_t shuffle, wrap;
    uint8_t fill[kChunkMaxElem];
};

// what the kernels know of an array ...
struct ChunkGeom {
    int32_t rank, es, unit, pad;
    int64_t E, stretch;               // elements of a chunk, of a stretch
    int32_t chunk[kChunkMaxRank];     // (a chunk is below 2 GiB)
    int64_t stride[kChunkMaxRank];    // of the array, in elements
    uint8_t fill[kChunkMaxElem];
};
// ... and of one chunk of it: its bytes, the array from the chunk's first element on, the extent that exists on every axis
struct ChunkJob {
    uint8_t *chunk, *arr;
    int32_t geom, flags;
    int32_t ext[kChunkMaxRank];
};

ZS_HD bool chunk_mul(int64_t a, int64_t b, int64_t *r) { return !__builtin_mul_overflow(a, b, r); }
ZS_HD int64_t chunk_ceil_div(int64_t a, int64_t b) { return a / b + (a % b != 0); }

// The rules of a grid; n_chunks, chunk_bytes and array_bytes where it keeps them.
ZS_HD bool chunk_grid_check(const ChunkGrid &g, int64_t *n_chunks, int64_t *chunk_bytes, int64_t *array_bytes) {
    if (g.rank < 1 || g.rank > kChunkMaxRank || g.elem_size < 1 || g.elem_size > kChunkMaxElem) return false;
    if (g.shuffle < 0 || g.shuffle > 1 || g.wrap < 0 || g.wrap > 2) return false;
    int64_t n = 1, cb = g.elem_size, ab = g.elem_size;
    for (int d = 0; d < g.rank; d++) {
        if (g.shape[d] < 1 || g.chunk[d] < 1) return false;
        if (!chunk_mul(n, chunk_ceil_div(g.shape[d], g.chunk[d]), &n) || !chunk_mul(cb, g.chunk[d], &cb) || !chunk_mul(ab, g.shape[d], &ab)) return false;
    }
    *n_chunks = n, *chunk_bytes = cb, *array_bytes = ab;
    return true;
}

// lane unit by the length of a chunk's row: 16 elements a lane where that keeps half a wave busy, else 4, else 1
ZS_HD int chunk_unit(int64_t row) { return row >= 512 ? 16 : row >= 64 ? 4 : 1; }

// (the grid has passed chunk_grid_check, and its chunk is at most kChunkMaxBytes)
ZS_HD ChunkGeom chunk_geom(const ChunkGrid &g) {
    ChunkGeom m;
    memset(&m, 0, sizeof m);
    m.rank = g.rank, m.es = g.elem_size, m.unit = chunk_unit(g.chunk[g.rank - 1]);
    m.stretch = 64 * kChunkPasses * m.unit, m.E = 1;
    int64_t s = 1;
    for (int d = g.rank - 1; d >= 0; d--) m.chunk[d] = (int32_t)g.chunk[d], m.E *= g.chunk[d], m.stride[d] = s, s *= g.shape[d];
    for (int j = 0; j < kChunkMaxElem; j++) m.fill[j] = g.fill[j];
    return m;
}

// Chunk c of the grid: its first element in the array (in elements), and the extent of it that exists on every axis.
ZS_HD int64_t chunk_place_of(const ChunkGrid &g, int64_t c, int32_t ext[kChunkMaxRank]) {
    int64_t origin = 0, s = 1;
    for (int d = g.rank - 1; d >= 0; d--) {
        const int64_t cells = chunk_ceil_div(g.shape[d], g.chunk[d]), p = c % cells, at = p * g.chunk[d];
        c /= cells;
        ext[d] = (int32_t)(g.shape[d] - at < g.chunk[d] ? g.shape[d] - at : g.chunk[d]);
        origin += at * s, s *= g.shape[d];
    }
    for (int d = g.rank; d < kChunkMaxRank; d++) ext[d] = 1;
    return origin;
}

// A chunk's items: its rows times the stretches of a row -- of the rows that exist, clipped (place, survey), or with `full`
// of all of them at full length (gather, which writes the padding).
ZS_HD int64_t chunk_item_count(const ChunkGeom &g, const int32_t ext[kChunkMaxRank], bool full) {
    const int32_t *dims = full ? g.chunk : ext;
    int64_t rows = 1;
    for (int d = 0; d + 1 < g.rank; d++) rows *= dims[d];
    return rows * chunk_ceil_div(dims[g.rank - 1], g.stretch);
}

struct ChunkItem {
    int64_t c_off, a_off;  // the stretch's first element: in the chunk, and in the array counted from the chunk's first
    int32_t n, n_exist;    // its elements, and how many of them (the first ones) exist in the array
};
ZS_HD ChunkItem chunk_item(const ChunkGeom &g, const int32_t ext[kChunkMaxRank], bool full, int64_t q) {
    const int32_t *dims = full ? g.chunk : ext;
    const int last = g.rank - 1;
    const int64_t n_str = chunk_ceil_div(dims[last], g.stretch);
    int64_t row = q / n_str, c_off = 0, a_off = 0, cs = g.chunk[last];
    const int64_t e0 = (q % n_str) * g.stretch;
    bool exists = true;
    for (int d = last - 1; d >= 0; d--) {
        const int64_t at = row % dims[d];
        row /= dims[d];
        c_off += at * cs, a_off += at * g.stride[d], cs *= g.chunk[d];
        exists = exists && at < ext[d];
    }
    ChunkItem it;
    it.c_off = c_off + e0, it.a_off = a_off + e0;
    it.n = (int32_t)(dims[last] - e0 < g.stretch ? dims[last] - e0 : g.stretch);
    const int64_t left = exists ? ext[last] - e0 : 0;
    it.n_exist = (int32_t)(left < 0 ? 0 : left < it.n ? left : it.n);
    return it;
}

// ---- 16 and 4 bytes at any address: one global_load / global_store_dwordx4 (dword) on the device (the unaligned-vector
// idiom of zs_tiff.hip), memcpy on the host
#if defined(__HIP_DEVICE_COMPILE__)
typedef uint32_t chunk_u32x4 __attribute__((ext_vector_type(4)));
typedef chunk_u32x4 chunk_u32x4_a1 __attribute__((aligned(1)));
typedef uint32_t chunk_u32_a1 __attribute__((aligned(1)));
#endif
ZS_HD void chunk_ld16(const uint8_t *p, uint32_t w[4]) {
#if defined(__HIP_DEVICE_COMPILE__)
    const chunk_u32x4 v = *(const chunk_u32x4_a1 *)p;
    w[0] = v.x, w[1] = v.y, w[2] = v.z, w[3] = v.w;
#else
    memcpy(w, p, 16);
#endif
}
ZS_HD void chunk_st16(uint8_t *p, const uint32_t w[4]) {
#if defined(__HIP_DEVICE_COMPILE__)
    chunk_u32x4 v;
    v.x = w[0], v.y = w[1], v.z = w[2], v.w = w[3];
    *(chunk_u32x4_a1 *)p = v;
#else
    memcpy(p, w, 16);
#endif
}
ZS_HD uint32_t chunk_ld4(const uint8_t *p) {
#if defined(__HIP_DEVICE_COMPILE__)
    return *(const chunk_u32_a1 *)p;
#else
    uint32_t v;
    memcpy(&v, p, 4);
    return v;
#endif
}
ZS_HD void chunk_st4(uint8_t *p, uint32_t v) {
#if defined(__HIP_DEVICE_COMPILE__)
    *(chunk_u32_a1 *)p = v;
#else
    memcpy(p, &v, 4);
#endif
}
template <int N>  // N words, 16 bytes at a time as far as they go
ZS_HD void chunk_ld_words(const uint8_t *p, uint32_t *w) {
#pragma unroll
    for (int k = 0; k < N; k += 4) {
        if (k + 4 <= N) {
            chunk_ld16(p + 4 * k, w + k);
        } else {
#pragma unroll
            for (int i = k; i < N; i++) w[i] = chunk_ld4(p + 4 * i);
        }
    }
}
template <int N>
ZS_HD void chunk_st_words(uint8_t *p, const uint32_t *w) {
#pragma unroll
    for (int k = 0; k < N; k += 4) {
        if (k + 4 <= N) {
            chunk_st16(p + 4 * k, w + k);
        } else {
#pragma unroll
            for (int i = k; i < N; i++) chunk_st4(p + 4 * i, w[i]);
        }
    }
}
ZS_HD uint32_t chunk_byte(const uint32_t *w, int b) { return (w[b >> 2] >> (8 * (b & 3))) & 255u; }

// ---- a lane's unit of U whole elements of ES bytes: U bytes of each plane (16: one 16-byte load a plane) interleaved in
// registers and written as U * ES contiguous bytes, 16 at a time; and the inverse
// (swap: the chunk's elements are big-endian -- plane j holds byte ES - 1 - j of the little-endian element)
template <int ES, int U>
ZS_HD void chunk_place_unit(const uint8_t *planes, int64_t E, uint8_t *out, bool swap = false) {
    constexpr int W = U / 4;
    uint32_t in[ES][W], o[ES * W];
#pragma unroll
    for (int j = 0; j < ES; j++) chunk_ld_words<W>(planes + (swap ? ES - 1 - j : j) * E, in[j]);
#pragma unroll
    for (int k = 0; k < ES * W; k++) {
        uint32_t v = 0;
#pragma unroll
        for (int b = 0; b < 4; b++) v |= chunk_byte(in[(4 * k + b) % ES], (4 * k + b) / ES) << (8 * b);
        o[k] = v;
    }
    chunk_st_words<ES * W>(out, o);
}
template <int ES, int U>
ZS_HD void chunk_gather_unit(const uint8_t *in, uint8_t *planes, int64_t E, bool swap = false) {
    constexpr int W = U / 4;
    uint32_t a[ES * W], o[W];
    chunk_ld_words<ES * W>(in, a);
#pragma unroll
    for (int j = 0; j < ES; j++) {
#pragma unroll
        for (int k = 0; k < W; k++) {
            uint32_t v = 0;
#pragma unroll
            for (int b = 0; b < 4; b++) v |= chunk_byte(a, (4 * k + b) * ES + j) << (8 * b);
            o[k] = v;
        }
        chunk_st_words<W>(planes + (swap ? ES - 1 - j : j) * E, o);
    }
}

// ---- a lane's share of a stretch of n elements: every 64th unit from its own on; the unit that the stretch ends in, byte by byte
template <int ES, int U>
ZS_HD void chunk_place_stretch(const uint8_t *planes, int64_t E, uint8_t *out, int n, int lane, bool swap = false) {
    for (int e = lane * U; e < n; e += 64 * U) {
        if (e + U <= n) {
            chunk_place_unit<ES, U>(planes + e, E, out + (int64_t)e * ES, swap);
        } else {
            for (int i = e; i < n; i++)
                for (int j = 0; j < ES; j++) out[(int64_t)i * ES + j] = planes[(swap ? ES - 1 - j : j) * E + i];
        }
    }
}
// (first n_exist elements from the array, the others `fill`)
template <int ES, int U>
ZS_HD void chunk_gather_stretch(const uint8_t *in, uint8_t *planes, int64_t E, int n, int n_exist, const uint8_t *fill, int lane, bool swap = false) {
    for (int e = lane * U; e < n; e += 64 * U) {
        if (e + U <= n_exist) {
            chunk_gather_unit<ES, U>(in + (int64_t)e * ES, planes + e, E, swap);
        } else {
            for (int i = e; i < n && i < e + U; i++)
                for (int j = 0; j < ES; j++) planes[(swap ? ES - 1 - j : j) * E + i] = i < n_exist ? in[(int64_t)i * ES + j] : fill[j];
        }
    }
}
// any element size, an element a lane and pass
ZS_HD void chunk_place_stretch_any(const uint8_t *planes, int64_t E, int es, uint8_t *out, int n, int lane, bool swap = false) {
    for (int i = lane; i < n; i += 64)
        for (int j = 0; j < es; j++) out[(int64_t)i * es + j] = planes[(swap ? es - 1 - j : j) * E + i];
}
ZS_HD void chunk_gather_stretch_any(const uint8_t *in, uint8_t *planes, int64_t E, int es, int n, int n_exist, const uint8_t *fill, int lane, bool swap = false) {
    for (int i = lane; i < n; i += 64)
        for (int j = 0; j < es; j++) planes[(swap ? es - 1 - j : j) * E + i] = i < n_exist ? in[(int64_t)i * es + j] : fill[j];
}

// 16 bytes of the fill pattern from byte b of a run of elements on
ZS_HD void chunk_fill16(const uint8_t *fill, int es, int b, uint32_t w[4]) {
    w[0] = w[1] = w[2] = w[3] = 0;
    int j = b % es;
#pragma unroll
    for (int i = 0; i < 16; i++) {
        w[i >> 2] |= (uint32_t)fill[j] << (8 * (i & 3));
        j = j + 1 == es ? 0 : j + 1;
    }
}
// 16 bytes that hold whole elements of es = 2, 4 or 8 bytes, every element's bytes reversed
ZS_HD void chunk_swap16(uint32_t w[4], int es) {
    if (es == 2) {
#pragma unroll
        for (int k = 0; k < 4; k++) w[k] = ((w[k] & 0x00FF00FFu) << 8) | ((w[k] >> 8) & 0x00FF00FFu);
    } else {
#pragma unroll
        for (int k = 0; k < 4; k++) w[k] = __builtin_bswap32(w[k]);
        if (es == 8) {
            uint32_t t = w[0];
            w[0] = w[1], w[1] = t, t = w[2], w[2] = w[3], w[3] = t;
        }
    }
}
// ---- the plain forms, over the bytes of a stretch, 16 a lane and pass: bytes [0, n_copy) copied, [n_copy, n) the fill pattern;
// swap (es 2, 4 or 8; the stretch and n_copy are whole elements): every element written with its bytes reversed
ZS_HD void chunk_copy_fill_stretch(const uint8_t *in, uint8_t *out, int n, int n_copy, const uint8_t *fill, int es, int lane, bool swap = false) {
    for (int b = lane * 16; b < n; b += 64 * 16) {
        uint32_t w[4];
        if (b + 16 <= n_copy) {
            chunk_ld16(in + b, w);
            if (swap) chunk_swap16(w, es);
            chunk_st16(out + b, w);
        } else if (b >= n_copy && b + 16 <= n) {
            chunk_fill16(fill, es, b, w);
            if (swap) chunk_swap16(w, es);
            chunk_st16(out + b, w);
        } else {
            for (int i = b; i < n && i < b + 16; i++) {
                const int k = swap ? i - i % es + (es - 1 - i % es) : i;  // the byte of the little-endian side that lands at i
                out[i] = i < n_copy ? in[k] : fill[k % es];
            }
        }
    }
}
// whether the lane's bytes of a stretch of n bytes are the fill pattern
ZS_HD bool chunk_is_fill_stretch(const uint8_t *in, int n, const uint8_t *fill, int es, int lane) {
    bool same = true;
    for (int b = lane * 16; b < n; b += 64 * 16) {
        if (b + 16 <= n) {
            uint32_t w[4], f[4];
            chunk_ld16(in + b, w);
            chunk_fill16(fill, es, b, f);
            same = same && w[0] == f[0] && w[1] == f[1] && w[2] == f[2] && w[3] == f[3];
        } else {
            for (int i = b; i < n; i++) same = same && in[i] == fill[i % es];
        }
    }
    return same;
}

// ---- one lane's work on item q of a job: KN's three kernels are these, a wave an item
#define ZS_CHUNK_UNITS(FN, ES, ...)                  \
    if (g.unit == 16) FN<ES, 16>(__VA_ARGS__);       \
    else FN<ES, 4>(__VA_ARGS__)

// place: the stretch's planes interleaved into the array (plain bytes copied; a job without bytes: the fill pattern)
ZS_HD void chunk_place_item(const ChunkGeom &g, const ChunkJob &jb, int64_t q, int lane) {
    const ChunkItem it = chunk_item(g, jb.ext, false, q);
    uint8_t *out = jb.arr + it.a_off * g.es;
    const bool swap = (jb.flags & kJobSwap) != 0;
    if (jb.flags & kJobFill) {
        chunk_copy_fill_stretch(out, out, it.n * g.es, 0, g.fill, g.es, lane);
    } else if (jb.flags & kJobPlain) {
        chunk_copy_fill_stretch(jb.chunk + it.c_off * g.es, out, it.n * g.es, it.n * g.es, g.fill, g.es, lane, swap);
    } else {
        const uint8_t *planes = jb.chunk + it.c_off;
        if (g.unit == 1 || !(g.es == 2 || g.es == 4 || g.es == 8)) {
            chunk_place_stretch_any(planes, g.E, g.es, out, it.n, lane, swap);
        } else if (g.es == 2) {
            ZS_CHUNK_UNITS(chunk_place_stretch, 2, planes, g.E, out, it.n, lane, swap);
        } else if (g.es == 4) {
            ZS_CHUNK_UNITS(chunk_place_stretch, 4, planes, g.E, out, it.n, lane, swap);
        } else {
            ZS_CHUNK_UNITS(chunk_place_stretch, 8, planes, g.E, out, it.n, lane, swap);
        }
    }
}
// gather: the inverse over the whole chunk, what does not exist in the array written as `fill`
ZS_HD void chunk_gather_item(const ChunkGeom &g, const ChunkJob &jb, int64_t q, int lane) {
    const ChunkItem it = chunk_item(g, jb.ext, true, q);
    const uint8_t *in = jb.arr + it.a_off * g.es;
    const bool swap = (jb.flags & kJobSwap) != 0;
    if (jb.flags & kJobPlain) {
        chunk_copy_fill_stretch(in, jb.chunk + it.c_off * g.es, it.n * g.es, it.n_exist * g.es, g.fill, g.es, lane, swap);
    } else {
        uint8_t *planes = jb.chunk + it.c_off;
        if (g.unit == 1 || !(g.es == 2 || g.es == 4 || g.es == 8)) {
            chunk_gather_stretch_any(in, planes, g.E, g.es, it.n, it.n_exist, g.fill, lane, swap);
        } else if (g.es == 2) {
            ZS_CHUNK_UNITS(chunk_gather_stretch, 2, in, planes, g.E, it.n, it.n_exist, g.fill, lane, swap);
        } else if (g.es == 4) {
            ZS_CHUNK_UNITS(chunk_gather_stretch, 4, in, planes, g.E, it.n, it.n_exist, g.fill, lane, swap);
        } else {
            ZS_CHUNK_UNITS(chunk_gather_stretch, 8, in, planes, g.E, it.n, it.n_exist, g.fill, lane, swap);
        }
    }
}
// survey: whether the lane's share of the item's existing elements is `fill`
ZS_HD bool chunk_survey_item(const ChunkGeom &g, const ChunkJob &jb, int64_t q, int lane) {
    const ChunkItem it = chunk_item(g, jb.ext, false, q);
    return chunk_is_fill_stretch(jb.arr + it.a_off * g.es, it.n * g.es, g.fill, g.es, lane);
}

// ================================================================== the filters beside shuffle (zs_chunk_filters)
struct ChunkFilters {  // zs_chunk_filters
    int32_t delta, byte_order, fletcher32, reserved;
};
// every field 0 or 1, reserved 0; delta and big-endian elements need an element of 1, 2, 4 or 8 bytes
ZS_HD bool chunk_filters_check(int elem_size, const ChunkFilters &f) {
    if (f.delta < 0 || f.delta > 1 || f.byte_order < 0 || f.byte_order > 1 || f.fletcher32 < 0 || f.fletcher32 > 1 || f.reserved != 0) return false;
    const bool pow2 = elem_size == 1 || elem_size == 2 || elem_size == 4 || elem_size == 8;
    return pow2 || !(f.delta || f.byte_order);
}

// ---- Fletcher-32 as HDF5 computes it (H5_checksum_fletcher32), in closed form: over the big-endian 16-bit words w_0 .. w_(N-1)
// of the bytes (an odd last byte is a word with a zero low byte), s1 = sum w_i and s2 = sum (N - i) w_i, both modulo 65535, a
// residue of 0 reading as 0xffff unless every word is zero.  A tile's pair (a1, a2) over its own n words, followed by m more
// words with the pair (b1, b2), combines to (a1 + b1, a2 + m a1 + b2).
constexpr int kFletTile = 16384;  // bytes of a tile (even: every tile but a span's last is whole words)
struct FletSum {
    uint32_t a1, a2, nz, pad;  // both below 65535; whether a byte of the words was not zero
};
struct FletSpan {
    const uint8_t *src;
    uint8_t *dst;  // where the four bytes of the checksum go, little-endian (may be null)
    int64_t len;
};
ZS_HD FletSum fletcher_combine(const FletSum &a, const FletSum &b, int64_t m_words) {
    FletSum r;
    r.a1 = (a.a1 + b.a1) % 65535u;
    r.a2 = (uint32_t)(((uint64_t)a.a2 + (uint64_t)(m_words % 65535) * a.a1 + b.a2) % 65535u);
    r.nz = a.nz | b.nz, r.pad = 0;
    return r;
}
ZS_HD uint32_t fletcher_finish(const FletSum &s) {
    const uint32_t s1 = s.a1 ? s.a1 : (s.nz ? 0xFFFFu : 0u), s2 = s.a2 ? s.a2 : (s.nz ? 0xFFFFu : 0u);
    return (s2 << 16) | s1;
}
ZS_HD int64_t fletcher_tiles(int64_t len) { return (len + kFletTile - 1) / kFletTile; }

// One 16-byte word of a tile as a lane meets it: byte i of it is byte p0 + i of the tile (p0 = 16 m - h may be negative in the
// tile's first word; bytes outside [0, len) do not count).  Adds the word's share of (sum w, sum (n - index) w) over the tile's
// n words to A1, A2: at most 2^20 and 2^34 a word, so a lane's 64-bit sums hold any tile.
ZS_HD void fletcher_word(const uint32_t w[4], int p0, int len, int n, uint64_t *A1, uint64_t *A2) {
    const int odd = p0 & 1, wi0 = (p0 - odd) / 2;  // the word index of byte p0's word (p0 - odd is even, also below 0)
    const bool full = p0 >= 0 && p0 + 16 <= len;
    uint32_t S = 0, T = 0;
#pragma unroll
    for (int i = 0; i < 16; i++) {
        uint32_t v = chunk_byte(w, i) << (((i ^ odd) & 1) ? 0 : 8);
        if (!full && (p0 + i < 0 || p0 + i >= len)) v = 0;
        S += v, T += (uint32_t)((i + odd) >> 1) * v;
    }
    *A1 += S;
    *A2 += (uint64_t)((int64_t)(n - wi0) * (int64_t)S - (int64_t)T);  // (every byte that counts has an index below n)
}
// a lane's share of a tile of len bytes that begins h bytes into the aligned word `base` points at: words lane, lane + 64, ...
ZS_HD void fletcher_tile_lane(const uint8_t *base, int h, int len, int lane, uint64_t *A1, uint64_t *A2) {
    const int n = (len + 1) / 2, words = (h + len + 15) >> 4;
    for (int m = lane; m < words; m += 64) {
        uint32_t w[4];
        chunk_ld16(base + 16 * (int64_t)m, w);
        fletcher_word(w, 16 * m - h, len, n, A1, A2);
    }
}

// ---- delta (numcodecs Delta over the whole padded chunk): enc[0] = x[0], enc[k] = x[k] - x[k-1], wrapping on elem_size bytes
constexpr int kDeltaUnit = 16, kDeltaPasses = 4;
constexpr int kDeltaTile = 64 * kDeltaUnit * kDeltaPasses;  // elements of a tile, a wave's work
enum { kDeltaShuffled = 1, kDeltaSwap = 2 };                // of a job's chunk side: in planes; elements big-endian
struct DeltaJob {
    const uint8_t *in;
    uint8_t *out;
    int64_t E;                 // elements
    int32_t es, flags, left;   // left: bytes behind the elements, copied unchanged (a bare buffer's len % elem_size)
    int32_t pad;
};
ZS_HD int64_t delta_tiles(int64_t E, int left) { return E ? (E + kDeltaTile - 1) / kDeltaTile : (left ? 1 : 0); }

// cnt <= 16 elements from element e on, as little-endian values: of a chunk side (flags: in planes of E bytes, plane j byte j of
// the stored element; big-endian) or, flags 0, of plain little-endian elements
template <int ES>
ZS_HD void delta_load(const uint8_t *p, int64_t E, int flags, int64_t e, int cnt, uint64_t x[kDeltaUnit]) {
    const bool sh = (flags & kDeltaShuffled) && ES > 1, swap = (flags & kDeltaSwap) && ES > 1;
#pragma unroll
    for (int k = 0; k < kDeltaUnit; k++) x[k] = 0;
    if (cnt == kDeltaUnit && sh) {
#pragma unroll
        for (int j = 0; j < ES; j++) {
            uint32_t w[4];
            chunk_ld16(p + (int64_t)(swap ? ES - 1 - j : j) * E + e, w);
#pragma unroll
            for (int k = 0; k < kDeltaUnit; k++) x[k] |= (uint64_t)chunk_byte(w, k) << (8 * j);
        }
    } else if (cnt == kDeltaUnit) {
        uint32_t w[4 * ES];
        chunk_ld_words<4 * ES>(p + e * ES, w);
#pragma unroll
        for (int k = 0; k < kDeltaUnit; k++)
#pragma unroll
            for (int j = 0; j < ES; j++) x[k] |= (uint64_t)chunk_byte(w, k * ES + (swap ? ES - 1 - j : j)) << (8 * j);
    } else {
        for (int k = 0; k < cnt; k++)
            for (int j = 0; j < ES; j++) {
                const int sj = swap ? ES - 1 - j : j;
                x[k] |= (uint64_t)(sh ? p[(int64_t)sj * E + e + k] : p[(e + k) * ES + sj]) << (8 * j);
            }
    }
}
template <int ES>
ZS_HD void delta_store(uint8_t *p, int64_t E, int flags, int64_t e, int cnt, const uint64_t x[kDeltaUnit]) {
    const bool sh = (flags & kDeltaShuffled) && ES > 1, swap = (flags & kDeltaSwap) && ES > 1;
    if (cnt == kDeltaUnit && sh) {
#pragma unroll
        for (int j = 0; j < ES; j++) {
            uint32_t w[4] = {0, 0, 0, 0};
#pragma unroll
            for (int k = 0; k < kDeltaUnit; k++) w[k >> 2] |= (uint32_t)((x[k] >> (8 * j)) & 255u) << (8 * (k & 3));
            chunk_st16(p + (int64_t)(swap ? ES - 1 - j : j) * E + e, w);
        }
    } else if (cnt == kDeltaUnit) {
        uint32_t w[4 * ES];
#pragma unroll
        for (int i = 0; i < 4 * ES; i++) w[i] = 0;
#pragma unroll
        for (int k = 0; k < kDeltaUnit; k++)
#pragma unroll
            for (int j = 0; j < ES; j++) {
                const int b = k * ES + (swap ? ES - 1 - j : j);
                w[b >> 2] |= (uint32_t)((x[k] >> (8 * j)) & 255u) << (8 * (b & 3));
            }
        chunk_st_words<4 * ES>(p + e * ES, w);
    } else {
        for (int k = 0; k < cnt; k++)
            for (int j = 0; j < ES; j++) {
                const int sj = swap ? ES - 1 - j : j;
                (sh ? p[(int64_t)sj * E + e + k] : p[(e + k) * ES + sj]) = (uint8_t)(x[k] >> (8 * j));
            }
    }
}
// the elements of pass `pass` of tile t that lane `lane` holds: from *e on, 0 .. 16 of them
ZS_HD int delta_lane_span(int64_t E, int64_t t, int pass, int lane, int64_t *e) {
    *e = t * kDeltaTile + ((int64_t)pass * 64 + lane) * kDeltaUnit;
    const int64_t left = E - *e;
    return left <= 0 ? 0 : left < kDeltaUnit ? (int)left : kDeltaUnit;
}
// encode, one lane's elements of one pass: x[k] - x[k-1] from the plain elements of jb.in into jb.out's chunk side
template <int ES>
ZS_HD void delta_encode_lane(const DeltaJob &jb, int64_t t, int pass, int lane) {
    int64_t e;
    const int cnt = delta_lane_span(jb.E, t, pass, lane, &e);
    if (cnt == 0) return;
    uint64_t x[kDeltaUnit], d[kDeltaUnit], prev = 0;
    delta_load<ES>(jb.in, jb.E, 0, e, cnt, x);
    if (e > 0)
        for (int j = 0; j < ES; j++) prev |= (uint64_t)jb.in[(e - 1) * ES + j] << (8 * j);
#pragma unroll
    for (int k = 0; k < kDeltaUnit; k++) d[k] = x[k] - (k ? x[k - 1] : prev);
    delta_store<ES>(jb.out, jb.E, jb.flags, e, cnt, d);
}
// decode: a lane's elements of one pass from the chunk side, and their sum (pass 1 needs no more) ...
template <int ES>
ZS_HD uint64_t delta_decode_load(const DeltaJob &jb, int64_t t, int pass, int lane, uint64_t x[kDeltaUnit], int64_t *e, int *cnt) {
    *cnt = delta_lane_span(jb.E, t, pass, lane, e);
    uint64_t sum = 0;
    if (*cnt == 0) return 0;
    delta_load<ES>(jb.in, jb.E, jb.flags, *e, *cnt, x);
#pragma unroll
    for (int k = 0; k < kDeltaUnit; k++) sum += x[k];  // (elements behind cnt are 0)
    return sum;
}
// ... and, pass 2, its running sums from `before` (everything in front of the lane's first element) on, written plain
template <int ES>
ZS_HD void delta_decode_store(const DeltaJob &jb, int64_t e, int cnt, uint64_t x[kDeltaUnit], uint64_t before) {
    if (cnt == 0) return;
#pragma unroll
    for (int k = 0; k < kDeltaUnit; k++) before += x[k], x[k] = before;
    delta_store<ES>(jb.out, jb.E, 0, e, cnt, x);
}
// the bytes behind the elements, by the lanes of the job's last tile
ZS_HD void delta_copy_left(const DeltaJob &jb, int64_t t, int lane) {
    if (t + 1 == delta_tiles(jb.E, jb.left) && lane < jb.left) jb.out[jb.E * jb.es + lane] = jb.in[jb.E * jb.es + lane];
}

}  // namespace zs
