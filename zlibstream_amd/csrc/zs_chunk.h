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
#pragma once

#include <cstdint>
#include <cstring>

#include "zs_core.h"

namespace zs {

constexpr int kChunkMaxRank = 8, kChunkMaxElem = 16;
constexpr int64_t kChunkMaxBytes = 0x7FFFFFFF - 1024;  // a chunk, in one call of the engine
constexpr int kChunkPasses = 4;                        // passes of the wave over a stretch

enum { kChunkStored = 1, kChunkUnshuffled = 2, kChunkSkip = 4, kChunkAbsent = 8 };  // ZS_CHUNK_*
enum { kJobPlain = 1, kJobFill = 2 };  // a job's bytes are not shuffled; it has none: its region is `fill`

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
template <int ES, int U>
ZS_HD void chunk_place_unit(const uint8_t *planes, int64_t E, uint8_t *out) {
    constexpr int W = U / 4;
    uint32_t in[ES][W], o[ES * W];
#pragma unroll
    for (int j = 0; j < ES; j++) chunk_ld_words<W>(planes + j * E, in[j]);
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
ZS_HD void chunk_gather_unit(const uint8_t *in, uint8_t *planes, int64_t E) {
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
        chunk_st_words<W>(planes + j * E, o);
    }
}

// ---- a lane's share of a stretch of n elements: every 64th unit from its own on; the unit that the stretch ends in, byte by byte
template <int ES, int U>
ZS_HD void chunk_place_stretch(const uint8_t *planes, int64_t E, uint8_t *out, int n, int lane) {
    for (int e = lane * U; e < n; e += 64 * U) {
        if (e + U <= n) {
            chunk_place_unit<ES, U>(planes + e, E, out + (int64_t)e * ES);
        } else {
            for (int i = e; i < n; i++)
                for (int j = 0; j < ES; j++) out[(int64_t)i * ES + j] = planes[j * E + i];
        }
    }
}
// (first n_exist elements from the array, the others `fill`)
template <int ES, int U>
ZS_HD void chunk_gather_stretch(const uint8_t *in, uint8_t *planes, int64_t E, int n, int n_exist, const uint8_t *fill, int lane) {
    for (int e = lane * U; e < n; e += 64 * U) {
        if (e + U <= n_exist) {
            chunk_gather_unit<ES, U>(in + (int64_t)e * ES, planes + e, E);
        } else {
            for (int i = e; i < n && i < e + U; i++)
                for (int j = 0; j < ES; j++) planes[j * E + i] = i < n_exist ? in[(int64_t)i * ES + j] : fill[j];
        }
    }
}
// any element size, an element a lane and pass
ZS_HD void chunk_place_stretch_any(const uint8_t *planes, int64_t E, int es, uint8_t *out, int n, int lane) {
    for (int i = lane; i < n; i += 64)
        for (int j = 0; j < es; j++) out[(int64_t)i * es + j] = planes[j * E + i];
}
ZS_HD void chunk_gather_stretch_any(const uint8_t *in, uint8_t *planes, int64_t E, int es, int n, int n_exist, const uint8_t *fill, int lane) {
    for (int i = lane; i < n; i += 64)
        for (int j = 0; j < es; j++) planes[j * E + i] = i < n_exist ? in[(int64_t)i * es + j] : fill[j];
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
// ---- the plain forms, over the bytes of a stretch, 16 a lane and pass: bytes [0, n_copy) copied, [n_copy, n) the fill pattern
ZS_HD void chunk_copy_fill_stretch(const uint8_t *in, uint8_t *out, int n, int n_copy, const uint8_t *fill, int es, int lane) {
    for (int b = lane * 16; b < n; b += 64 * 16) {
        uint32_t w[4];
        if (b + 16 <= n_copy) {
            chunk_ld16(in + b, w);
            chunk_st16(out + b, w);
        } else if (b >= n_copy && b + 16 <= n) {
            chunk_fill16(fill, es, b, w);
            chunk_st16(out + b, w);
        } else {
            for (int i = b; i < n && i < b + 16; i++) out[i] = i < n_copy ? in[i] : fill[i % es];
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
    if (jb.flags & kJobFill) {
        chunk_copy_fill_stretch(out, out, it.n * g.es, 0, g.fill, g.es, lane);
    } else if (jb.flags & kJobPlain) {
        chunk_copy_fill_stretch(jb.chunk + it.c_off * g.es, out, it.n * g.es, it.n * g.es, g.fill, g.es, lane);
    } else {
        const uint8_t *planes = jb.chunk + it.c_off;
        if (g.unit == 1 || !(g.es == 2 || g.es == 4 || g.es == 8)) {
            chunk_place_stretch_any(planes, g.E, g.es, out, it.n, lane);
        } else if (g.es == 2) {
            ZS_CHUNK_UNITS(chunk_place_stretch, 2, planes, g.E, out, it.n, lane);
        } else if (g.es == 4) {
            ZS_CHUNK_UNITS(chunk_place_stretch, 4, planes, g.E, out, it.n, lane);
        } else {
            ZS_CHUNK_UNITS(chunk_place_stretch, 8, planes, g.E, out, it.n, lane);
        }
    }
}
// gather: the inverse over the whole chunk, what does not exist in the array written as `fill`
ZS_HD void chunk_gather_item(const ChunkGeom &g, const ChunkJob &jb, int64_t q, int lane) {
    const ChunkItem it = chunk_item(g, jb.ext, true, q);
    const uint8_t *in = jb.arr + it.a_off * g.es;
    if (jb.flags & kJobPlain) {
        chunk_copy_fill_stretch(in, jb.chunk + it.c_off * g.es, it.n * g.es, it.n_exist * g.es, g.fill, g.es, lane);
    } else {
        uint8_t *planes = jb.chunk + it.c_off;
        if (g.unit == 1 || !(g.es == 2 || g.es == 4 || g.es == 8)) {
            chunk_gather_stretch_any(in, planes, g.E, g.es, it.n, it.n_exist, g.fill, lane);
        } else if (g.es == 2) {
            ZS_CHUNK_UNITS(chunk_gather_stretch, 2, in, planes, g.E, it.n, it.n_exist, g.fill, lane);
        } else if (g.es == 4) {
            ZS_CHUNK_UNITS(chunk_gather_stretch, 4, in, planes, g.E, it.n, it.n_exist, g.fill, lane);
        } else {
            ZS_CHUNK_UNITS(chunk_gather_stretch, 8, in, planes, g.E, it.n, it.n_exist, g.fill, lane);
        }
    }
}
// survey: whether the lane's share of the item's existing elements is `fill`
ZS_HD bool chunk_survey_item(const ChunkGeom &g, const ChunkJob &jb, int64_t q, int lane) {
    const ChunkItem it = chunk_item(g, jb.ext, false, q);
    return chunk_is_fill_stretch(jb.arr + it.a_off * g.es, it.n * g.es, g.fill, g.es, lane);
}

}  // namespace zs
